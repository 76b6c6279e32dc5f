"""The device reservoir sample (pepper_amd/csrc/encoder.hip: reservoir_keep_kernel behind pa_encoder_set_sampling) on the
hand-built piles of tests/sampling_cases.py: the parallel regeneration and what carries over between regenerations, the mask
at small i, the loops of stride 256, the rank-to-pair scan over dead pairs, k = int(min(cap, rate * n)) in double, five
intervals in one launch, and the clearing of a dropped pair.

Every expected value is the reference's loop on numpy.random.RandomState (sampling_cases.numpy_slots) over the pattern the case
plans, which tests/test_sampling_cases_cpu.py recomputes; none comes from the package's own sampler.  Integer work: bit-exact.
Per case, one small BAM through PackedEncoder.pack + encode: the planned pattern with sampling off, the kept pairs and
live[r] == k with it on, sampled() advanced by exactly the sampled intervals and their dropped reads, and the first result back
with it off again.  Downstream, a sampled interval's results -- every array of the variant encoder, rows / reads / chunks of the
polish chain with and without re-alignment -- equal those of a BAM that holds only the reads the oracle keeps: a dropped pair is
left exactly as a pair that keeps nothing.  pair_live reads the variant encoder's pair table, which a chain run does not fill:
the polish tests compare reads per region and the arrays only.

Wall time of the module on an MI355X: 3.6 s for its 71 tests, 1.5 s of it the first handle; the slowest case (cap_edge /
n10003) takes 0.3 s.

Which cases fail under which deliberate break of the kernel (scratch builds, never committed; every break stays inside the
kernel's buffers and ends), one run of this module per build, and whether tests/test_gpu_device_sampling.py (its handle test and
the image-file comparisons of both pipelines, run in the same builds) noticed:
    (a) the second stretch of the regeneration starts on word 228: 20 failures -- 9 of the 13 cases of regen_boundary,
        mask / k3_every_power_of_two, stride (n = 2k + 3, k7 from n = 511), cap_edge / n10003, ranks / k40, the two downstream
        variant cases that draw that far.  The k = 1 and k = 7 samples that end within a word of the first regeneration keep
        their slots: the one wrong word they draw moves none.  The older module noticed (4 of 4).
    (b) mt[kk] written in front of the barrier: nothing fails, here or in the older module.  The barrier orders three pairs of
        words per stretch across wavefronts (kk = 63 | 64, 127 | 128, 191 | 192; within a wavefront every lane has read before any
        writes); at one workgroup of four wavefronts the read wins that race every time.  No test of results can force the order.
    (c) `at` restarting on word 1 of every regeneration but the first (carried over as it is, `at` would be 624, no word would
        be drawn and the loop would not end: that form was not run): 9 failures -- regen_boundary / k1_ends_on_1247,
        k1_opens_third, k255_two_rejections_close (also downstream), mask / k3, stride / k7 from n = 511, cap_edge / n10003.
        The older module noticed on the variant side only (2 of 4).
    (d) + (e) + (f) in one build -- `carry` not added in the rank scan, `flags &= READ_REV` removed, (float)rate * n: 45 failures.
        (f) alone explains rate / p29_of_100 and p57_of_100 (100 pairs: one pass, no carry; k = 29 and 57); (d) every case of more
        than 256 pairs, all of ranks among them.  The older module noticed (4 of 4; not separated into (d) and (f)).
    (e) alone: nothing fails, here or in the older module, and nothing can: with ncig = 0 a pair that kept READ_MAPQ_OK is
        walked over no operation by segment_reads_kernel / tile_count_kernel and by the polish encoder alike.  The clearing of
        the flag is a second lock on the same door; what the downstream tests pin is that the pair contributes nothing.
    (g) `v <= i` turned into `v < i`: 44 failures -- every family but many, the small i of mask (k1_n2 .. n5) and rate
        (half_of_2, half_of_3) first of all, and all four polish runs.  The older module did NOT notice (4 of 4 passed): at i >= 5000 a
        word equal to i is one in 8192."""
import numpy as np
import pytest

import bam_utils as bu
import sampling_cases as sc

pytestmark = pytest.mark.gpu

PARAMS = (1, 1, 0.1, 0.15, 0.15, 3, 0.1, 0.12, 2, False)
KEYS = {"images", "positions", "depths", "candidates", "candidate_frequency"}
REF = sc.reference()
FAR = dict(pos=8000, reverse=False, mapq=60, seq=REF[8000:8030], qual=np.full(30, 30, np.uint8), cigar=[(0, 30)], name="far")


@pytest.fixture(scope="module")
def packed():
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    enc = PackedEncoder(0, arena_bytes=16 << 20)
    yield enc
    enc.close()


def _bam(tmp_path, name, reads):
    from pepper_amd.variant.bam import BAM_handler
    path = str(tmp_path / (name + ".bam"))
    bu.write_bam(path, [("ctg", len(REF))], {0: reads}, flush_every=47)
    return BAM_handler(path)


def _encode(enc, handler, case, sampling, only=None):
    """pack + encode of the case's intervals (only: of that one alone) -> (results per interval, reads per interval, the
    intervals' pair offsets, pair_live over all pairs)."""
    bounds, windows = sc.bounds(case), [(a, b) for a, b, _ in case.intervals]
    if only is not None:
        bounds, windows = [bounds[only]], [windows[only]]
    n = len(bounds)
    n_done, region_pairs, counts = enc.pack(handler, "ctg", [lo for lo, _ in bounds], [hi for _, hi in bounds], False, 1)
    assert n_done == n
    outs, live = enc.encode(bounds, [REF[lo:hi + 1] for lo, hi in bounds], region_pairs, counts, PARAMS, windows, sampling=sampling)
    offsets = [int(x) for x in region_pairs[:n + 1]]
    return outs, [int(x) for x in live], offsets, enc.pair_live(offsets[n]).copy()


def _same_results(got, want, what):
    assert set(got) == set(want) and KEYS <= set(want), what
    for key in want:
        g, w = got[key], want[key]
        if w is None:                    # (the int32 images, which these calls do not ask for)
            assert g is None, (what, key)
            continue
        assert (g == w) if isinstance(w, (list, bytes)) else (g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)), (what, key)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_ids())
def test_kept_pairs_counters_and_switching_off(case, packed, tmp_path):
    handler = _bam(tmp_path, "case", sc.reads_of(case))
    sampling = (case.seed, case.cap, case.rate)
    # the planned pattern, sampling off
    plain, live0, offsets, pairs0 = _encode(packed, handler, case, None)
    for r, (_a, _b, pattern) in enumerate(case.intervals):
        got = "".join("L" if x else "D" for x in pairs0[offsets[r]:offsets[r + 1]])
        assert got == pattern, (r, got)
        assert live0[r] == pattern.count("L") == case.expect["n"][r]
    # the kept set, sampling on
    before = packed.sampled()
    outs, live1, offsets1, pairs1 = _encode(packed, handler, case, sampling)
    assert offsets1 == offsets
    sampled = dropped = 0
    for r, n in enumerate(live0):
        seg0, seg1 = pairs0[offsets[r]:offsets[r + 1]], pairs1[offsets[r]:offsets[r + 1]]
        k = sc.allowed(case.cap, case.rate, n)
        if n <= k:
            assert case.expect["k"][r] is None and live1[r] == n and np.array_equal(seg1, seg0), r
            _same_results(outs[r], plain[r], ("not sampled", r))
            continue
        assert case.expect["k"][r] == k == live1[r], (r, live1[r])
        ranks = np.flatnonzero(seg0)                             # rank among the interval's reads -> pair of the interval
        want = sorted(ranks[sc.numpy_slots(case.seed, n, k)].tolist())
        assert np.flatnonzero(seg1).tolist() == want, r
        sampled, dropped = sampled + 1, dropped + n - k
    # the counters
    assert (sampled, dropped) == case.expect["sampled"]
    assert packed.sampled() == (before[0] + sampled, before[1] + dropped)
    # off again: nothing lingers in the handle
    again, live2, offsets2, pairs2 = _encode(packed, handler, case, None)
    assert live2 == live0 and offsets2 == offsets and np.array_equal(pairs2, pairs0)
    assert packed.sampled() == (before[0] + sampled, before[1] + dropped)
    for r in range(len(live0)):
        _same_results(again[r], plain[r], ("off again", r))


@pytest.mark.parametrize("key", sc.DOWNSTREAM_VARIANT, ids=lambda key: "%s-%s" % key)
def test_variant_results_equal_those_of_the_kept_reads_alone(key, packed, tmp_path):
    """Every interval of the call under sampling against an encode of that interval alone from a BAM that holds only the reads
    the oracle keeps of it (and one read far behind every interval, so that the file is never empty): images, positions, depths,
    candidates, candidate frequencies.  A dropped pair that kept a flag, an operation or a base would show here."""
    case = sc.case(*key)
    handler = _bam(tmp_path, "all", sc.reads_of(case))
    plain, live0, _offsets, _pairs = _encode(packed, handler, case, None)
    outs, live, _offsets, _pairs = _encode(packed, handler, case, (case.seed, case.cap, case.rate))
    changed = with_candidates = 0
    for r in range(len(case.intervals)):
        kept = sc.kept_reads(case, r)
        alone, live_alone, _o, pairs_alone = _encode(packed, _bam(tmp_path, "kept%d" % r, kept + [FAR]), case, None, only=r)
        assert live_alone == [len(kept)] == [live[r]] and int(pairs_alone.sum()) == len(kept), r
        _same_results(outs[r], alone[0], (key, r))
        if case.expect["k"][r] is not None:
            changed += not np.array_equal(outs[r]["images"], plain[r]["images"]) or outs[r]["candidates"] != plain[r]["candidates"]
            with_candidates += len(outs[r]["candidates"]) > 0
            assert len(plain[r]["candidates"]) > 0, r
    assert changed == case.expect["sampled"][0] > 0                        # (the sample shows in what is compared)
    assert with_candidates > 0 or all(k in (None, 0) for k in case.expect["k"])


@pytest.mark.parametrize("realign", [True, False], ids=["realign", "no_realign"])
@pytest.mark.parametrize("key", sc.DOWNSTREAM_POLISH, ids=lambda key: "%s-%s" % key)
def test_polish_chain_equals_that_of_the_kept_reads_alone(key, realign, packed, tmp_path):
    """PolishChain.run(..., sampling=(seed, cap)) against a run without sampling over the kept-only BAM: rows, reads per region,
    chunks per region and the chunk arrays (images, positions, indices)."""
    from pepper_amd.polish.PEPPER import PolishChain
    case = sc.case(*key)
    assert case.rate == 1.0 and len(case.intervals) == 1
    chain, bounds = PolishChain(packed), sc.bounds(case)
    windows = [REF[lo:hi + 20].encode() for lo, hi in bounds]

    def run(handler, sampling):
        n_done, region_pairs, counts = packed.pack(handler, "ctg", [lo for lo, _ in bounds], [hi for _, hi in bounds], False, 0)
        assert n_done == len(bounds)
        rows, live, chunks = chain.run(bounds, windows, region_pairs, counts, realign=realign, chunk_size=200, chunk_overlap=50,
                                       sampling=sampling)
        return rows.tolist(), live.tolist(), chunks.tolist(), [a.copy() for a in chain.chunk_arrays()]
    try:
        before = packed.sampled()
        got = run(_bam(tmp_path, "all", sc.reads_of(case)), (case.seed, case.cap))
        assert packed.sampled() == (before[0] + case.expect["sampled"][0], before[1] + case.expect["sampled"][1])
        want = run(_bam(tmp_path, "kept", sc.kept_reads(case, 0) + [FAR]), None)
        plain = run(_bam(tmp_path, "all", sc.reads_of(case)), None)
    finally:
        packed.set_sampling(None)
    assert got[1] == [n if k is None else k for n, k in zip(case.expect["n"], case.expect["k"])]
    assert got[:3] == want[:3] and sum(got[2]) == len(got[3][0]) > 1 and got[0][0] > 0
    for g, w in zip(got[3], want[3]):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    assert plain[1] == case.expect["n"] and not (plain[3][0].shape == got[3][0].shape and np.array_equal(plain[3][0], got[3][0]))
