"""The polish summary encoder's kernels (pepper_amd/csrc/encoder_polish.hip) on the hand-built pileups of
tests/polish_encoder_cases.py: tile edges, 64-operation passes, the scans' carries across 1 024, buffers that outgrow their
first sizes, the two "runs past its sequence" errors, spans that differ from the region; host-fed (generate_summary,
generate_summaries, StagedSummaries, a handle of the test's own) and device-fed (PolishChain.run over a BAM, chunked).  The
expectation is the restatement, which tests/test_polish_encoder_cases_cpu.py pins to the reference build on exactly these cases
(and the reference build itself for the device-fed form).  Integer work: bit-exact, no tolerances.

The unmodified kernels pass every case: no bug was found.  Deliberate breaks, each tried once on a scratch copy of
encoder_polish.hip against this module (not committed; all three only drop counted work):
    - the second `put` of polish_segment_kernel removed (the record of an insert in front of a read's first aligned base for
      the previous tile): 8 tests failed -- test_every_case_and_span_in_a_call_of_its_own[tile_edges] and [spans],
      test_a_family_as_one_batch_equals_region_by_region[tile_edges] and [spans], test_staged_batch_run_twice and the three
      cases of test_buffers_outgrown_on_a_new_handle (through the three-tile pileups on the grown handle).  The device-fed
      tests cannot see it: the clipping drops an insert in front of the first aligned base.
    - `first <= stop` -> `first < stop` in polish_segment_kernel: 12 failed -- the single calls of tile_edges, spans,
      scan_edges and many_regions, the batches of tile_edges, spans and scan_edges, test_many_regions_as_one_call,
      test_staged_batch_run_twice, the three cases of test_buffers_outgrown_on_a_new_handle
    - `live_max = tile_hi` instead of `tile_hi + 1` in polish_tile_kernel: 15 failed -- the single calls and the batches of
      tile_edges, many_operations, spans and scan_edges, test_staged_batch_run_twice, the three cases of
      test_buffers_outgrown_on_a_new_handle, test_operations_past_the_sequence_are_errors_and_the_handle_goes_on,
      test_device_fed_chain_equals_the_reference_build, test_chunk_edges"""
import ctypes

import numpy as np
import pytest

import bam_utils as bu
import pileup_utils as pu
import polish_encoder_cases as pc
from conftest import need_reference_build
from pepper_amd import _lib

pytestmark = pytest.mark.gpu

BATCH_FAMILIES = ("by_hand", "tile_edges", "many_operations", "spans", "scan_edges", "staircase")
_families, _want, _single = {}, {}, {}


def family(name):
    if name not in _families:
        _families[name] = pc.FAMILIES[name]()
    return _families[name]


def items_of(name):
    """[(key, case, (start, end))] of a family: every case under every one of its spans."""
    return [((name, cname, k), case, span) for cname, case in family(name).items() for k, span in enumerate(case[4])]


def want(key, case, span):
    """The restatement's rows: computed once per case and span, never changed."""
    if key not in _want:
        img, pos = pu.run_polish_oracle(pu.load_restatement(), pc.pileup(case), *span)
        img.flags.writeable = pos.flags.writeable = False
        _want[key] = (img, pos)
    return _want[key]


def flat_of(pile):
    return dict(read_pos=pile.read_pos, read_reverse=pile.read_reverse, read_mapq=pile.read_mapq, seq_offset=pile.seq_offset,
                seq=pile.seq, qual=pile.qual, cigar_offset=pile.cigar_offset, cigar_op=pile.cigar_op, cigar_len=pile.cigar_len,
                n_reads=pile.n_reads)


def single(key, case, span):
    """One region through SummaryGenerator.generate_summary (the thread's handle), once per case and span."""
    from pepper_amd.polish.PEPPER import SummaryGenerator
    if key not in _single:
        gen = SummaryGenerator(case[2], "contig_1", case[0], case[1])
        gen.generate_summary(flat_of(pc.pileup(case)), *span)
        _single[key] = (gen.image, gen.positions_array)
    return _single[key]


def same(got, exp, what):
    assert got[0].shape == exp[0].shape and got[1].shape == exp[1].shape, what
    assert np.array_equal(got[1], exp[1]), what
    assert np.array_equal(got[0], exp[0]), what


# ---- host-fed: single calls -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.FAMILIES))
def test_every_case_and_span_in_a_call_of_its_own(name):
    for key, case, span in items_of(name):
        same(single(key, case, span), want(key, case, span), key)
    if name == "tile_edges":       # the wrap quirk is in what was compared: 2 forward gaps over coverage 0 -> 508 & 0xff
        img, pos = want(("tile_edges", "gaps", 0), family(name)["gaps"], family(name)["gaps"][4][0])
        assert (img[[r for r in pc.DELETION_ONLY_ROWS]] == np.array([0] * 8 + [254, 252], np.uint8)).all()
        assert (pos[pc.DELETION_ONLY_ROWS[0]] == (pc.R0 + pc.DELETION_ONLY_ROWS[0], 0)).all()


# ---- host-fed: batches ----------------------------------------------------------------------------------------------------------
def _empty_case(k):
    """A region without reads: 1, 513 or 700 rows of zeros."""
    R, L = 200_000 + 1_000 * k, (1, 513, 700)[k % 3]
    return (("empty", k, 0), (R, R + L - 1, pc.reference(R, L), [], [(R, R + L - 1)]), (R, R + L - 1))


def _batch(items):
    from pepper_amd.polish.PEPPER import SummaryGenerator, generate_summaries
    gens = [SummaryGenerator(case[2], "contig_1", case[0], case[1]) for _, case, _ in items]
    generate_summaries(gens, [flat_of(pc.pileup(case)) for _, case, _ in items], [span for _, _, span in items])
    return [(g.image, g.positions_array) for g in gens]


def _check_batch(items, what):
    got = _batch(items)
    assert len(got) == len(items)
    for g, (key, case, span) in zip(got, items):
        same(g, single(key, case, span), (what, key))
        same(g, want(key, case, span), (what, key))


@pytest.mark.parametrize("name", BATCH_FAMILIES)
def test_a_family_as_one_batch_equals_region_by_region(name):
    items = items_of(name)
    _check_batch(items, "in order")
    _check_batch(items[::-1], "reversed")
    spaced = [_empty_case(0)]
    for k, it in enumerate(items):
        spaced += [it, _empty_case(k + 1)]
    _check_batch(spaced, "with empty regions")


def test_many_regions_as_one_call():
    """1 100 regions = 1 100 tiles in one call: polish_bases_kernel and polish_tile_offsets_kernel take a second block of
    1 024, and regions 1 022 .. 1 026 and the last one have insert rows that a lost carry would move."""
    items = items_of("many_regions")
    assert len(items) == 1100
    got = _batch(items)
    n_ins = 0
    for g, (key, case, span) in zip(got, items):
        same(g, single(key, case, span), key)
        same(g, want(key, case, span), key)
        n_ins += int((g[1][:, 1] > 0).sum())
    assert n_ins >= 2 * len(pc.INSERT_REGIONS)


def test_staged_batch_run_twice():
    from pepper_amd.polish.PEPPER import StagedSummaries, SummaryGenerator
    items = items_of("tile_edges")
    gens = [SummaryGenerator(case[2], "contig_1", case[0], case[1]) for _, case, _ in items]
    flats = [flat_of(pc.pileup(case)) for _, case, _ in items]
    staged = StagedSummaries(gens, flats, [span for _, _, span in items])
    for attempt in range(2):
        rows = staged.run().copy()
        img, pos = staged.results()
        stats = staged.stats()
        assert stats["regions"] == len(items) and stats["rows"] == int(rows.sum()) and stats["runs"] >= 1 and stats["tiles"] == 4 * len(items)
        at = 0
        for n, (key, case, span) in zip(rows.tolist(), items):
            same((img[at:at + n], pos[at:at + n]), want(key, case, span), (attempt, key))
            at += n
        assert at == len(img)


# ---- a handle of the test's own ---------------------------------------------------------------------------------------------------
class Handle(object):
    """pa_encoder_create through ctypes: its buffers have seen nothing, so their first sizes are really the first."""

    def __init__(self):
        self.lib = _lib.load()
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.pa_encoder_create(0, None, ctypes.byref(self.h)))

    def close(self):
        self.lib.pa_encoder_destroy(self.h)

    def batch(self, piles, spans):
        from pepper_amd.variant.PEPPER_VARIANT import _Pileup
        n = len(piles)
        structs = (_Pileup * n)(*[_Pileup(p.region_start, p.region_end, p.reference, len(p.reference), p.n_reads, p.read_pos.ctypes.data,
                                          p.read_reverse.ctypes.data, p.read_mapq.ctypes.data, p.seq_offset.ctypes.data, p.seq.ctypes.data,
                                          p.qual.ctypes.data, p.cigar_offset.ctypes.data, p.cigar_op.ctypes.data, p.cigar_len.ctypes.data)
                                  for p in piles])
        starts = np.array([s for s, _ in spans], np.int64)
        ends = np.array([e for _, e in spans], np.int64)
        rows = np.zeros(n, np.int64)
        _lib.check(self.lib.pa_polish_encoder_generate_summary_batch(self.h, n, ctypes.cast(structs, ctypes.c_void_p), starts.ctypes.data,
                                                                     ends.ctypes.data, rows.ctypes.data))
        total = int(rows.sum())
        img, pos = np.zeros((total, 10), np.uint8), np.zeros((total, 2), np.int64)
        _lib.check(self.lib.pa_polish_encoder_get_results(self.h, img.ctypes.data, pos.ctypes.data))
        cuts = np.concatenate([[0], np.cumsum(rows)]).tolist()
        return [(img[a:b], pos[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]

    def runs(self):
        v = np.zeros(8, np.int64)
        _lib.check(self.lib.pa_polish_encoder_batch_stats(self.h, v.ctypes.data, 8))
        assert v[7] == 0
        return int(v[6])

    def check(self, items, what):
        got = self.batch([pc.pileup(case) for _, case, _ in items], [span for _, _, span in items])
        for g, (key, case, span) in zip(got, items):
            same(g, want(key, case, span), (what, key))


@pytest.fixture
def handle():
    h = Handle()
    yield h
    h.close()


@pytest.mark.parametrize("which", ["long_inserts", "many_records", "both"])
def test_buffers_outgrown_on_a_new_handle(handle, which):
    """6 000 insert slots where the first size is 2 * 200 + 4 096; ~2 300 tile records where it is bases / 512 + 2 * reads +
    1 024 (tests/test_polish_encoder_cases_cpu.py checks both inequalities): the call is run again with room, which the seventh
    value of pa_polish_encoder_batch_stats shows; then the three-tile pileups on the grown handle, in one run."""
    items = [it for it in items_of("capacity") if which in (it[0][1], "both")]
    assert len(items) == (2 if which == "both" else 1)
    handle.check(items, which)
    assert handle.runs() >= 2, handle.runs()
    handle.check(items, which + " again")
    assert handle.runs() == 1
    handle.check(items_of("tile_edges"), "tile_edges on the grown handle")
    assert handle.runs() == 1


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def _lengthened(case, kind):
    """The case's pileup with one operation lengthened past the read's bases -> (pileup, index of the read)."""
    pile = pc.pileup(case)
    for k, r in enumerate(case[3]):
        ops = [op for op, _ in r["cigar"]]
        if kind == pc.M and r["cigar"][0] == (pc.M, 600) and 0 <= r["pos"] - case[0] < 1024:
            pile.cigar_len[int(pile.cigar_offset[k])] += 100_000
            return pile, k
        if kind == pc.I and ops == [pc.M, pc.I, pc.M] and r["pos"] > case[0] + 400:
            pile.cigar_len[int(pile.cigar_offset[k]) + 1] += 50
            return pile, k
    raise AssertionError("no such read")


def test_operations_past_the_sequence_are_errors_and_the_handle_goes_on(handle):
    te = family("tile_edges")
    good = [it for it in items_of("tile_edges") if it[0][1] in ("gaps", "odd_bases")]
    for kind, cname, word in ((pc.M, "first_m", "CIGAR"), (pc.I, "inner_inserts", "insert")):
        case = te[cname]
        bad, k = _lengthened(case, kind)
        assert k > 0
        with pytest.raises(_lib.PepperAmdError, match=r"%s of read %d runs past its sequence" % (word, k)) as err:
            handle.batch([bad], [case[4][0]])
        assert err.value.code == _lib.PA_ERR_INVALID and "of region" not in str(err.value)
        handle.check(good, "after the refused call")
        # in a batch: behind a region with reads and one without, the read is counted inside its own region
        piles = [pc.pileup(good[0][1]), pc.pileup(_empty_case(0)[1]), bad, pc.pileup(good[1][1])]
        spans = [good[0][2], _empty_case(0)[2], case[4][0], good[1][2]]
        with pytest.raises(_lib.PepperAmdError, match=r"%s of read %d of region 2 runs past its sequence" % (word, k)):
            handle.batch(piles, spans)
        handle.check([(("tile_edges", cname, 0), case, case[4][0])] + good, "after the refused batch")


# ---- device-fed: the image chain over a BAM -----------------------------------------------------------------------------------------
BAM_LETTERS = set("=ACMGRSVTWYHKDBN")


def _bam_reads():
    """The reads of tile_edges and many_operations as a BAM can hold them: upper case, none with N / P operations (the restated
    clipping does not cover them) or with a base outside the BAM alphabet."""
    reads = list(family("tile_edges")["all"][3])
    for case in family("many_operations").values():
        reads += case[3]
    out = []
    for r in reads:
        seq = r["seq"].upper()
        if any(op in (pc.N, pc.P) for op, _ in r["cigar"]) or not set(seq) <= BAM_LETTERS:
            continue
        out.append(dict(r, seq=seq))
    out.sort(key=lambda r: r["pos"])
    for i, r in enumerate(out):
        r["name"] = "q%d" % i
    return out


def chunks_of(img, pos, chunk_size, overlap):
    """chunk_images of the reference's AlignmentSummarizer.py:18-56 as a plain loop: chunk_size rows, the next chunk starting
    `overlap` rows before the end of this one, the last one padded with zero rows at position / index -1."""
    total, out = len(pos), []
    start, end = 0, min(len(pos), chunk_size)
    while True:
        ci, cp = np.zeros((chunk_size, 10), np.uint8), np.full((chunk_size, 2), -1, np.int64)
        ci[:end - start] = img[start:end]
        cp[:end - start] = pos[start:end]
        out.append((ci, cp, end - start))
        if end == total:
            break
        start = end - overlap
        end = min(total, start + chunk_size)
    return out


@pytest.fixture(scope="module")
def chain_rig(tmp_path_factory):
    """The BAM and draft on disk, the three regions packed once, and the reference build's rows for each region."""
    from pepper_amd.polish import PEPPER
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    from pepper_amd.variant.bam import BAM_handler
    ref_enc = pu.load_reference_polish_encoder()
    if ref_enc is None:
        need_reference_build("oracle/_ref (polish encoder)")
    tmp = tmp_path_factory.mktemp("polish_cases")
    R, L = pc.R0, pc.L0
    draft = pc.reference(0, R + L + 1200)
    reads = _bam_reads()
    assert len(reads) > 80 and max(len(r["cigar"]) for r in reads) == 200
    bam_path, fa_path = str(tmp / "reads.bam"), str(tmp / "draft.fa")
    bu.write_bam(bam_path, [("ctg1", len(draft))], {0: reads})
    with open(fa_path, "w") as fh:
        fh.write(">ctg1\n" + draft + "\n")
    bounds = [(R - 1000, R + 199), (R, R + L - 1), (R + L - 200, R + L + 999)]
    rows = []
    for a, b in bounds:
        clipped = bu.restated_get_reads(reads, a, b, False, 0)
        assert len(clipped) >= 10
        rows.append(pu.run_polish_reference(ref_enc, pu.FlatPileup(a, b, draft[a:b + 1], clipped), a, b))
    enc = PackedEncoder(0, 64 << 20, host_threads=1)
    n_done, region_pairs, counts = enc.pack(BAM_handler(bam_path), "ctg1", [a for a, _ in bounds], [b for _, b in bounds], False, 0)
    assert n_done == 3
    yield dict(chain=PEPPER.PolishChain(enc), bounds=bounds, rows=rows, region_pairs=region_pairs, counts=counts, reads=reads)
    enc.close()


def _run_chain(rig, chunk_size, overlap):
    chain, bounds = rig["chain"], rig["bounds"]
    n_rows, live, chunks = chain.run(bounds, [b"" for _ in bounds], rig["region_pairs"], rig["counts"], realign=False,
                                     chunk_size=chunk_size, chunk_overlap=overlap)
    img, pos, idx = [a.copy() for a in chain.chunk_arrays()]
    expect = [chunks_of(wi, wp, chunk_size, overlap) for wi, wp in rig["rows"]]
    assert n_rows.tolist() == [len(wi) for wi, _ in rig["rows"]]
    assert live.tolist() == [len(bu.restated_get_reads(rig["reads"], a, b, False, 0)) for a, b in bounds]
    assert chunks.tolist() == [len(e) for e in expect]
    assert img.shape == (sum(len(e) for e in expect), chunk_size, 10)         # no chunk follows the last
    at = 0
    for r, e in enumerate(expect):
        for c, (wi, wp, used) in enumerate(e):
            assert np.array_equal(pos[at], wp[:, 0]) and np.array_equal(idx[at], wp[:, 1]), (r, c)
            assert np.array_equal(img[at], wi), (r, c)
            # only a region's last chunk is padded: zero pixels, position / index -1
            assert used == chunk_size or c == len(e) - 1
            assert not img[at][used:].any() and (pos[at][used:] == -1).all() and (idx[at][used:] == -1).all() and (pos[at][:used] >= 0).all()
            at += 1
    return expect


def test_device_fed_chain_equals_the_reference_build(chain_rig):
    """The reads as unpack_clip_kernel leaves them (clipped on the device from BAM records: inserts on tile edges, 200-operation
    reads, deletions over tile starts, reads over both region edges) through the same kernels; the product's chunk shape."""
    expect = _run_chain(chain_rig, 1000, 50)
    assert [len(e) for e in expect] == [2, 2, 2]
    wi, wp = chain_rig["rows"][1]
    assert ((wp[:, 0] == pc.R0 + 511) & (wp[:, 1] > 0)).any() and ((wp[:, 0] == pc.R0 + 1023) & (wp[:, 1] > 0)).any()


def _chunk_pairs(nr):
    pairs = [(nr, 50), (nr - 1, 50), (nr + 1, 50), (1000, 50), (256, 0), (257, 256), (100, 99)]
    step = next(d for d in range(150, 1, -1) if (nr - 200) % d == 0)         # nr - chunk_size an exact multiple of chunk_size - overlap
    return pairs + [(200, 200 - step)]


def test_chunk_edges(chain_rig):
    nr = len(chain_rig["rows"][1][1])
    pairs = _chunk_pairs(nr)
    assert (nr - pairs[-1][0]) % (pairs[-1][0] - pairs[-1][1]) == 0 and nr > 1537
    for chunk_size, overlap in pairs:
        expect = _run_chain(chain_rig, chunk_size, overlap)
        n_mid = len(expect[1])
        assert n_mid == (1 if nr <= chunk_size else 1 + -(-(nr - chunk_size) // (chunk_size - overlap))), (chunk_size, overlap)
