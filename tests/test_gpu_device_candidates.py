"""Candidates enumerated on the device (pa_encoder_set_device_candidates: group_votes_kernel, enumerate_sites_kernel) against
the host enumeration of the same handle and the reference's own encoder build.  Every pile runs three ways -- switch on,
switch off, reference -- and every key must be equal: positions, depths, candidates, candidate_frequency, int8 and int32 images.
The handle's counters say where each call was enumerated."""
import os
import threading

import numpy as np
import pytest

import bam_utils as bu
import pileup_utils as pu
from test_encoder_oracle import CASES, PRESET_CASES, _case, preset_case
from test_gpu_encoder import _check, _gen_and_flat, _inner_region_case, _product, _tile_edge_case

pytestmark = pytest.mark.gpu

KEYS = ("positions", "depths", "candidate_frequency", "images", "images_int32")
SITE_MAX = 1024          # CAND_SITE_MAX of csrc/encoder.hip: the votes one site may have on the device path


@pytest.fixture(scope="module")
def ref_lib():
    lib = pu.load_reference_encoder()
    assert lib is not None, "oracle/_ref/libref_variant_encoder.so: the reference's own encoder build is the third way"
    return lib


def _equal(a, b):
    assert a["candidates"] == b["candidates"]
    for key in KEYS:
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key


def _on_and_off(run, calls=1, on_host=0):
    """run() with the switch off, then on: equal results; the counters move by the calls made, on the side expected."""
    from pepper_amd.variant import PEPPER_VARIANT as pv
    pv.set_device_candidates(False)
    before = pv.candidate_calls()
    off = run()
    assert pv.candidate_calls() == before                      # off: neither counter moves
    pv.set_device_candidates(True)
    try:
        on = run()
    finally:
        pv.set_device_candidates(False)
    after = pv.candidate_calls()
    assert (after[0] - before[0], after[1] - before[1]) == (calls - on_host, on_host)
    return on, off


def _three_ways(ref_lib, pile, params, on_host=0):
    on, off = _on_and_off(lambda: _product(pile, params), on_host=on_host)
    _equal(on, off)
    _check(on, pu.run_variant(ref_lib, pile, params, reference_impl=True))
    return on


# ---- existing families ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_named_families(ref_lib, name):
    got = _three_ways(ref_lib, *_case(**CASES[name]))
    assert len(got["candidates"]) > 0


def test_golden_vectors(ref_lib, golden_dir):
    names = [n for n in sorted(CASES) if os.path.exists(os.path.join(golden_dir, f"encoder_variant_{n}.npz"))]
    assert "deep_over_125" in names and len(names) >= 4
    for name in names:
        g = np.load(os.path.join(golden_dir, f"encoder_variant_{name}.npz"))
        got = _three_ways(ref_lib, *_case(**CASES[name]))
        assert got["candidates"] == [s for s in str(g["candidates"]).split("\n") if s]
        assert np.array_equal(got["images_int32"].astype(np.int16), g["images"])
        assert np.array_equal(got["positions"], g["positions"])


@pytest.mark.parametrize("preset,name", [("hifi", "low_quality_heavy"), ("clr", "indel_heavy"), ("ont_r10_q20", "deep")])
def test_reference_presets(ref_lib, preset, name):
    assert name in PRESET_CASES
    assert len(_three_ways(ref_lib, *preset_case(preset, name))["candidates"]) > 0


@pytest.mark.parametrize("case", [lambda: _tile_edge_case(1124, 1024), lambda: _tile_edge_case(613, 513),
                                  lambda: _inner_region_case(9, long_indel_rate=0.3, low_q_rate=0.4)])
def test_tile_edges_and_region_edges(ref_lib, case):
    assert len(_three_ways(ref_lib, *case())["candidates"]) > 0


# ---- hand-built piles -----------------------------------------------------------------------------------------------------
OFF = 20_000


def _read(ref, edits, reverse, lo=0, hi=None):
    """A read matching ref[lo:hi] but for `edits`: {row: ("S", base) | ("I", bases) | ("D", length)}, an indel following the
    aligned base on its row."""
    hi = len(ref) if hi is None else hi
    seq, cigar, at = [], [], lo

    def push(op, n):
        if n > 0:
            if cigar and cigar[-1][0] == op:
                cigar[-1] = (op, cigar[-1][1] + n)
            else:
                cigar.append((op, n))
    for row in sorted(edits):
        kind, what = edits[row]
        assert lo < row < hi - 70
        seq.append(ref[at:row])
        push(pu.OP_M, row - at)
        seq.append(what if kind == "S" else ref[row])
        push(pu.OP_M, 1)
        at = row + 1
        if kind == "I":
            seq.append(what)
            push(pu.OP_I, len(what))
        elif kind == "D":
            push(pu.OP_D, what)
            at += what
    seq.append(ref[at:hi])
    push(pu.OP_M, hi - at)
    s = "".join(seq)
    return dict(pos=OFF + lo, reverse=bool(reverse), mapq=30, seq=s, qual=np.full(len(s), 30, np.uint8), cigar=cigar)


def _pile(ref, reads, **over):
    reads = sorted(reads, key=lambda r: r["pos"])
    return pu.FlatPileup(OFF, OFF + len(ref) - 1, ref, reads), pu.make_params(OFF, OFF + len(ref) - 1, **over)


def _other(base):
    return "ACGT"[("ACGT".index(base) + 1) % 4]


LOOSE = dict(snp_candidate_freq_threshold=0.04, indel_candidate_freq_threshold=0.04, snp_freq_threshold=0.04,
             insert_freq_threshold=0.04, delete_freq_threshold=0.04)


def test_allele_order_past_the_first_eight_bytes(ref_lib):
    """An insert's key is its anchor base and the inserted bases: alleles that agree on their first 8 bytes and differ at byte 9
    or byte 20, strict prefixes at 8 / 9 and 20 / 21 bytes, a 61-byte key -- every one on both strands, two reads each, at one
    site.  At a second site deletions of 9, 12 and 20 bases (their tails lie in the reference, each a prefix of the next) beside
    inserts of 9 and 12 (tails in the pool); at a third a SNP, an insert and a deletion together."""
    rng = np.random.default_rng(41)
    ref = pu.random_reference(rng, 400)
    long = "".join(rng.choice(list("ACGT"), size=59))       # the longest allele the reference keeps: a key of 61 characters
    stem = long[:24]

    def flip(s, k):
        return s[:k] + _other(s[k]) + s[k + 1:]
    inserts = [stem[:20], flip(stem[:20], 7), flip(stem[:20], 8), flip(stem[:20], 18), flip(stem[:20], 19),
               stem[:7], stem[:8], stem[:19], stem[:21], stem[:3], long, flip(long, 58), long[:58]]
    assert len(set(inserts)) == len(inserts)
    reads = []
    for k, ins in enumerate(inserts):
        for rev in (0, 1):
            edits = {100: ("I", ins)}
            if k < 3:
                edits[200] = ("D", (9, 12, 20)[k])
            elif k < 5:
                edits[200] = ("I", ("GATTACAGA", "GATTACAGATTC")[k - 3])
            elif k < 7:
                edits[200] = ("D", 3)
            if k in (7, 8):
                edits[300] = ("S", _other(ref[300]))
            elif k in (9, 10):
                edits[300] = ("I", "TG")
            elif k in (11, 12):
                edits[300] = ("D", 11)
            reads.append(_read(ref, edits, rev))
    reads += [_read(ref, {}, k % 2) for k in range(40 - len(reads))]
    assert len(reads) == 40
    got = _three_ways(ref_lib, *_pile(ref, reads, **LOOSE))
    at = {p: [c for c, q in zip(got["candidates"], got["positions"]) if q == OFF + p] for p in (100, 200, 300)}
    assert len(at[100]) == len(inserts) and all(c[0] == "2" for c in at[100]) and max(len(c) for c in at[100]) == 61
    assert [c[0] for c in at[200]] == ["2", "2", "3", "3", "3", "3"] and [len(c) for c in at[200]][2:] == [5, 11, 14, 22]
    assert [c[0] for c in at[300]] == ["1", "2", "3"]
    assert (got["candidate_frequency"][got["positions"] == OFF + 100] == 2).all()


def _wide_site(n_votes, n_plain=4):
    """One site with n_votes reads that each carry one of three inserts, interleaved in read order, on short reads."""
    rng = np.random.default_rng(n_votes)
    ref = pu.random_reference(rng, 260)
    alleles = ("ACGTACGTTTGACA", "ACGTACGTTTGACC", "T")
    reads = [_read(ref, {100: ("I", alleles[k % 3])}, k % 2, lo=60 + k % 7, hi=200 - k % 5) for k in range(n_votes)]
    reads += [_read(ref, {}, k % 2) for k in range(n_plain)]
    return _pile(ref, reads)


@pytest.mark.parametrize("n_votes", [65, 128, 129])
def test_sites_of_more_votes_than_a_wavefront(ref_lib, n_votes):
    got = _three_ways(ref_lib, *_wide_site(n_votes))
    here = got["positions"] == OFF + 100
    assert here.sum() == 3 and (got["depths"][here] == min(125, n_votes + 4)).all()
    assert sorted(got["candidate_frequency"][here].tolist()) == sorted(min(125, len(range(k, n_votes, 3))) for k in range(3))


def test_site_at_the_bound_and_one_vote_past_it(ref_lib):
    """SITE_MAX votes at one site stay on the device; one more and the kernels refuse the call: the host enumerates it, the
    results are the same, and the host counter says so."""
    got = _three_ways(ref_lib, *_wide_site(SITE_MAX))
    assert (got["positions"] == OFF + 100).sum() == 3
    got = _three_ways(ref_lib, *_wide_site(SITE_MAX + 1), on_host=1)
    assert (got["positions"] == OFF + 100).sum() == 3


def _rare_pile(seed):
    rng = np.random.default_rng(seed)
    ref = pu.random_reference(rng, 300)
    reads = []
    for k in range(36):
        edits = {}
        if k < 8:
            edits[90] = ("S", "N" if k < 4 else _other(ref[90]))          # N beside an ACGT allele, both strands
        if 8 <= k < 20:
            edits[150] = ("S", ("n", "R", "Y", _other(ref[150]).lower())[k % 4])
        reads.append(_read(ref, edits, k % 2))
    return _pile(ref, reads, **LOOSE)


def test_rare_alphabet(ref_lib):
    """Read letters outside ACGT at SNP sites, beside ACGT alleles, on both strands, at two sites of one region -- and in two
    regions of one batch, enumerated on the device in one call: equal to the host's batch, to the regions one by one and to
    the reference's build."""
    pile, params = _rare_pile(51)
    got = _three_ways(ref_lib, pile, params)
    assert "1N" in got["candidates"] and "1R" in got["candidates"] and "1n" in got["candidates"]
    assert len(set(got["positions"][[c[1] not in "ACGT" for c in got["candidates"]]].tolist())) == 2
    cases = _shared([(pile, params), _case(**CASES["plain"]), _rare_pile(52)], **LOOSE)
    on, off = _on_and_off(lambda: _batch(cases))                  # one call: the device counter by 1, the host counter by 0
    singles = [_product(p, q) for p, q in cases]
    for k, (p, q) in enumerate(cases):
        _equal(on[k], off[k])
        _equal(on[k], singles[k])
        _check(on[k], pu.run_variant(ref_lib, p, q, reference_impl=True))
    for k in (0, 2):                                              # the rare chains of two regions at once
        rare = [c[1] not in "ACGT" for c in on[k]["candidates"]]
        assert len(set(on[k]["positions"][rare].tolist())) == 2


RARE = "NRYKMSWBDHVnrykmsw"          # eighteen read letters outside ACGT


def _many_letters(n_letters):
    """One SNP site where n_letters distinct letters outside ACGT each sit on three reads (both strands), and no ACGT allele."""
    ref = pu.random_reference(np.random.default_rng(300 + n_letters), 300)
    reads = [_read(ref, {140: ("S", RARE[k // 3])}, k % 2) for k in range(3 * n_letters)]
    reads += [_read(ref, {}, k % 2) for k in range(60 - len(reads))]
    return _pile(ref, reads, **LOOSE)


def test_more_rare_letters_than_a_site_holds(ref_lib):
    """A site holds SNP_MAX = 16 SNP alleles (csrc/candidates.h).  Sixteen distinct rare letters fill it and stay on the device,
    equal to the reference; with seventeen the kernels refuse the call (which letters the host's n_snp == 16 rule drops depends
    on its own order): the host enumerates it, the results are those of the switch off, and the host counter says so.  Such a
    site is no pileup, so the reference is not asked about it."""
    got = _three_ways(ref_lib, *_many_letters(16))
    assert sorted(c[1] for c in got["candidates"]) == sorted(RARE[:16]) and (got["candidate_frequency"] == 3).all()
    pile, params = _many_letters(17)
    on, off = _on_and_off(lambda: _product(pile, params), on_host=1)
    _equal(on, off)
    assert len(on["candidates"]) >= 16 and (on["positions"] == OFF + 140).all()


# ---- thresholds at equality -----------------------------------------------------------------------------------------------
def _counted(depth, n_alt, kind):
    rng = np.random.default_rng(1000 + depth)
    ref = pu.random_reference(rng, 260)
    edit = {"snp": ("S", _other(ref[120])), "ins": ("I", "GA"), "del": ("D", 2)}[kind]
    return ref, [_read(ref, {120: edit} if k < n_alt else {}, k % 2) for k in range(depth)]


@pytest.mark.parametrize("kind,over,depth,n_alt", [
    ("snp", dict(snp_candidate_freq_threshold=0.1, snp_freq_threshold=0.05), 30, 3),
    ("ins", dict(indel_candidate_freq_threshold=0.1, insert_freq_threshold=0.05), 30, 3),
    ("del", dict(indel_candidate_freq_threshold=0.1, delete_freq_threshold=0.05), 30, 3),
    ("ins", dict(candidate_support_threshold=4, indel_candidate_freq_threshold=0.01, insert_freq_threshold=0.05), 30, 4),
    ("snp", dict(candidate_support_threshold=4, snp_candidate_freq_threshold=0.01, snp_freq_threshold=0.05), 30, 4),
    ("snp", dict(snp_candidate_freq_threshold=0.1, snp_freq_threshold=0.05), 130, 13),
    ("del", dict(indel_candidate_freq_threshold=0.104, delete_freq_threshold=0.05), 130, 13),
])
def test_thresholds_at_equality(ref_lib, kind, over, depth, n_alt):
    """total / depth (the depth clamped to 125) exactly on a frequency threshold, support exactly on the support threshold, each
    beside its neighbour one read short: in on one side, out on the other, as the reference decides in double."""
    found = []
    for n in (n_alt, n_alt - 1):
        ref, reads = _counted(depth, n, kind)
        got = _three_ways(ref_lib, *_pile(ref, reads, **over))
        found.append(int((got["positions"] == OFF + 120).sum()))
    assert found == [1, 0]


def test_skip_indels(ref_lib):
    ref, reads = _counted(30, 10, "ins")
    reads = [_read(ref, {60: ("S", _other(ref[60]))} if k < 8 else {}, k % 2) for k in range(12)] + reads
    with_indels = _three_ways(ref_lib, *_pile(ref, reads))
    without = _three_ways(ref_lib, *_pile(ref, reads, skip_indels=1))
    assert [c[0] for c in with_indels["candidates"]] == ["1", "2"] and [c[0] for c in without["candidates"]] == ["1"]


# ---- batches --------------------------------------------------------------------------------------------------------------
RULES = ("min_snp_baseq", "min_indel_baseq", "snp_freq_threshold", "insert_freq_threshold", "delete_freq_threshold",
         "min_coverage_threshold", "snp_candidate_freq_threshold", "indel_candidate_freq_threshold", "candidate_support_threshold",
         "skip_indels")


def _shared(cases, **over):
    """The piles of `cases` under one set of thresholds, each with its own candidate region: a batch call takes one set for all
    of its regions."""
    return [(pile, pu.make_params(q.candidate_region_start, q.candidate_region_end, **over)) for pile, q in cases]


def _batch(cases):
    from pepper_amd.variant.PEPPER_VARIANT import generate_summary_arrays_batch
    p0 = cases[0][1]
    assert all(getattr(q, f) == getattr(p0, f) for _, q in cases for f in RULES), "one call, one set of thresholds"
    gens, flats = zip(*[_gen_and_flat(pile) for pile, _ in cases])
    return generate_summary_arrays_batch(
        list(gens), list(flats), p0.min_snp_baseq, p0.min_indel_baseq, p0.snp_freq_threshold, p0.insert_freq_threshold,
        p0.delete_freq_threshold, p0.min_coverage_threshold, p0.snp_candidate_freq_threshold, p0.indel_candidate_freq_threshold,
        p0.candidate_support_threshold, bool(p0.skip_indels), [(q.candidate_region_start, q.candidate_region_end) for _, q in cases],
        32, 26, False, want_int32=True)


def _quiet_cases():
    """Regions that give no candidate: without reads, without a passing site, with a passing site whose alleles all fall short."""
    rng = np.random.default_rng(61)
    ref = pu.random_reference(rng, 300)
    no_reads = _pile(ref, [])
    no_sites = _pile(ref, [_read(ref, {}, k % 2) for k in range(12)])
    alts = [c for c in "ACGT" if c != ref[150]]
    no_accepted = _pile(ref, [_read(ref, {150: ("S", alts[k])} if k < 3 else {}, k % 2) for k in range(30)])
    return [no_reads, no_sites, no_accepted]


@pytest.mark.parametrize("n_regions", [1, 2, 17])
def test_batches_equal_their_regions_one_by_one(ref_lib, n_regions):
    quiet = _quiet_cases()
    loud = [_case(**CASES["plain"]), _tile_edge_case(3, 700), _wide_site(70), _rare_pile(53), _case(**CASES["deep_over_125"])]
    if n_regions == 1:
        cases = [loud[0]]
    elif n_regions == 2:
        cases = [quiet[2], loud[1]]
    else:
        cases = [quiet[0], quiet[1], loud[0], loud[1], quiet[2], loud[2], quiet[0], loud[3], quiet[1], loud[4], loud[0], quiet[2],
                 loud[2], loud[1], quiet[1], quiet[2], quiet[0]]
    assert len(cases) == n_regions
    cases = _shared(cases, **LOOSE)
    on, off = _on_and_off(lambda: _batch(cases))
    assert sum(len(g["candidates"]) for g in on) > 0
    for k, (pile, params) in enumerate(cases):
        _equal(on[k], off[k])
        want = pu.run_variant(ref_lib, pile, params, reference_impl=True)
        assert len(want["candidates"]) > 0 or any(pile is q[0] for q in quiet)
        _check(on[k], want)
    singles, _ = _on_and_off(lambda: [_product(pile, params) for pile, params in cases], calls=n_regions)
    for one, many in zip(singles, on):
        _equal(many, one)


def test_all_quiet_batch(ref_lib):
    on, off = _on_and_off(lambda: _batch(_quiet_cases()))
    assert [len(g["candidates"]) for g in on] == [0, 0, 0] == [len(g["candidates"]) for g in off]


# ---- growth ---------------------------------------------------------------------------------------------------------------
def test_more_candidates_than_the_first_buffer_guess(ref_lib):
    """A new handle (a new thread has its own) sizes its candidate buffers for 1024: a small call, then one with several times
    that many candidates -- the kernels write nothing, the buffers grow and the call runs again -- then the small call again."""
    small = _case(**CASES["plain"])
    big = []
    for seed in (81, 82, 83):                  # a SNP on every other row in half of twelve reads: ~700 candidates a region
        ref = pu.random_reference(np.random.default_rng(seed), 1500)
        snps = {row: ("S", _other(ref[row])) for row in range(20, 1420, 2)}
        big.append(_pile(ref, [_read(ref, snps if k < 6 else {}, k % 2) for k in range(12)]))
    failures = []

    def body():
        try:
            first, _ = _on_and_off(lambda: _product(*small))
            on, off = _on_and_off(lambda: _batch(big))
            assert sum(len(g["candidates"]) for g in on) > 1024 + 512
            for k, (pile, params) in enumerate(big):
                _equal(on[k], off[k])
                _check(on[k], pu.run_variant(ref_lib, pile, params, reference_impl=True))
            again, _ = _on_and_off(lambda: _product(*small))
            _equal(again, first)
        except BaseException as err:       # noqa: B902 -- handed to the test's own thread
            failures.append(err)
    t = threading.Thread(target=body)
    t.start()
    t.join()
    if failures:
        raise failures[0]


# ---- the packed path ------------------------------------------------------------------------------------------------------
def test_packed_path(tmp_path):
    """PackedEncoder.pack_device + encode(resident=True, sampling=...) on a small BAM: switch on equals switch off, with an
    interval deep enough to be sampled down on the device in front of the enumeration."""
    from pepper_amd.variant.bam import BAM_handler
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    rng = np.random.default_rng(71)
    ref = pu.random_reference(rng, 16000)
    sites = {int(p): ("ACGT"[("ACGT".index(ref[p]) + 1) % 4], 0.5) for p in rng.choice(np.arange(300, 15000), 60, replace=False)}
    reads = pu.simulate_reads(rng, ref, 0, n_reads=500, read_len=(400, 3000), snp_sites=sites,
                              indel_sites={4000: ("I", "ACGTACGTTTGACA", 0.5), 9000: ("D", 12, 0.5)}, clip_rate=0.3)
    reads += pu.simulate_reads(rng, ref[6000:7500], 6000, n_reads=300, read_len=(600, 1400), snp_sites=sites)
    reads = sorted([r for r in reads if not any(op in (3, 6) for op, _ in r["cigar"])], key=lambda r: r["pos"])
    for i, r in enumerate(reads):
        r["name"] = "read_%05d" % i
    bam = str(tmp_path / "in.bam")
    bu.write_bam(bam, [("ctg", len(ref))], {0: reads}, flush_every=23)
    params = (1, 1, 0.1, 0.15, 0.15, 3, 0.1, 0.12, 2, False)
    edges = list(range(1000, 15001, 2000))
    starts, stops = [a - 100 for a in edges[:-1]], [b + 100 for b in edges[1:]]
    regions, refs, cands = list(zip(starts, stops)), [ref[a:b + 1] for a, b in zip(starts, stops)], list(zip(edges[:-1], edges[1:]))
    enc = PackedEncoder(0, arena_bytes=32 << 20)
    handler = BAM_handler(bam)
    out = {}
    for on in (False, True):
        enc.set_device_candidates(on)
        before = enc.candidate_calls()
        packed = enc.pack_device(handler, "ctg", starts, stops, False, 1)
        assert packed is not None and packed[0] == len(starts)
        out[on], live = enc.encode(regions, refs, packed[1], packed[2], params, cands, want_int32=True, resident=True,
                                   sampling=(2022, 150, 1.0))
        after = enc.candidate_calls()
        assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if on else (0, 0))
        assert live.max() == 150                   # the deep interval was sampled down
    enc.close()
    assert sum(len(g["candidates"]) for g in out[True]) > 40
    for g, w in zip(out[True], out[False]):
        _equal(g, w)
