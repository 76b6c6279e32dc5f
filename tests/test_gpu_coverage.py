"""pa_encoder_set_depth_bins through the C ABI: the depth classes of a run's positions, run-length encoded on the device.

Every expected value is Coverage.runs_numpy / totals_numpy of coverage_cases.depth_numpy over the reads the BAM was written
from; none comes from the code under test.

One batch of four regions of one contig with 300, 512, 513 and 1 500 positions (a partial tile, exactly the positions of one
tile, a second tile with one position, three tiles; each matrix has one more, all-zero, row), as tests/test_gpu_region_bed.py.
The reads are laid out by hand (positions relative to OFF):
  1000 - 1299   no read at all: one run of bin 0
  1400 - 1600   three reads; one of them has two bases of quality 0, the first rescued by the insert behind it (depth 3 / 2)
  1601 - 1700   two reads and one read of (1M1D) x 50: the depth alternates 3, 2 with every base -- a run per row
  1701 - 1799   nothing: a stretch of depth 0 inside a region
  1800 - 2000   five reads over the end of the 512-row region and the start of the 513-row one
  2001 - 2424   one read, two more with a deletion inside, four more over 2300 - 2423: the depth drops on 2424, the window's last
                row and row 0 of the second tile.  Four reads START on 2424, the fetch's end: a fetch of [a, b] takes the reads
                with pos < b (bam_handler.cpp's iterator is half-open; the image driver pads every fetch by 100 bases), so they
                are no reads of that region
  2600          row 0 of the 1 500-row region: nothing; 2601 - 3110 five reads (and one of mapping quality 0, which does not count);
  3111          row 511: two reads; 3112, row 512: nothing; 3113 - 3500 (from row 513) five reads; 3501 - 3700 nothing;
  3701 - 4098   six reads, one of which goes on to 4150: depth 1 on 4099, the last row
SNPs carried by two reads of a block give the runs candidates, so that `candidates and images unchanged` is not vacuous."""
import ctypes

import numpy as np
import pytest

import bam_utils as bu
import pileup_utils as pu
from coverage_cases import depth_numpy
from pepper_amd.variant import Coverage, Targets

pytestmark = pytest.mark.gpu

OFF = 350_000
CONTIG_LEN = 700_000
SPAN = 5000
REGIONS = [(OFF + 1000, OFF + 1299), (OFF + 1400, OFF + 1911), (OFF + 1912, OFF + 2424), (OFF + 2600, OFF + 4099)]
PARAMS = (1, 1, 0.1, 0.15, 0.15, 3, 0.1, 0.12, 2, False)
MIN_SNP_Q, MIN_INDEL_Q, MIN_COV = 1, 1, 3
BINS = [0, 1, MIN_COV]
KEYS = ("positions", "depths", "candidate_frequency", "images")
# the table of tests/test_gpu_region_bed.py: edges on rows 0, 511, 512 and 513 of the 1 500-row region, on the first and last
# row of the 513-row region, an interval of one base, one over the end of a region and the start of the next, none in the first
TARGETS = [(900, 950), (1500, 1600), (1900, 1913), (2415, 2425), (2600, 2610), (3100, 3112), (3113, 3130), (3500, 3501),
           (3600, 3900), (4200, 4300)]
SNPS = (1500, 1850, 2700, 3300, 3800)


def _read(ref, pos, cigar, name, alts=(), bad=(), mapq=60, reverse=False):
    """A read at OFF + pos whose aligned bases are the reference's but for `alts` (relative positions that carry another
    base); inserted and clipped bases are G; every quality is 30 but for the aligned bases at `bad` (0)."""
    seq, qual, p = [], [], pos
    for op, n in cigar:
        if op == pu.OP_M:
            for k in range(n):
                base = ref[p + k]
                seq.append("ACGT"[("ACGT".index(base) + 1) % 4] if p + k in alts else base)
                qual.append(0 if p + k in bad else 30)
            p += n
        elif op == pu.OP_D:
            p += n
        else:
            seq.extend("G" * n)
            qual.extend([30] * n)
    return dict(pos=OFF + pos, reverse=reverse, mapq=mapq, seq="".join(seq), qual=np.array(qual, np.uint8), cigar=list(cigar), name=name)


def build_job(directory):
    assert [b - a + 1 for a, b in REGIONS] == [300, 512, 513, 1500]
    ref = pu.random_reference(np.random.default_rng(9107), SPAN)
    M, I, D, S = pu.OP_M, pu.OP_I, pu.OP_D, pu.OP_S
    reads = []

    def block(k, lo, hi, snp=None, **kw):
        for j in range(k):
            reads.append(_read(ref, lo, [(M, hi - lo + 1)], "b%d_%d" % (lo, j), alts=(snp,) if snp is not None and j < 2 else (),
                               reverse=j % 2 == 1, **kw))
    reads.append(_read(ref, 1400, [(S, 5), (M, 51), (I, 2), (M, 150)], "rescued", bad=(1450, 1460)))
    block(2, 1400, 1600, snp=1500)
    block(2, 1601, 1700)
    reads.append(_read(ref, 1601, [(M, 1), (D, 1)] * 50, "comb"))
    block(5, 1800, 2000, snp=1850)
    block(1, 2001, 2424)
    block(4, 2300, 2423)
    for j in range(2):
        reads.append(_read(ref, 2100, [(M, 50), (D, 10), (M, 41)], "gap%d" % j, reverse=bool(j)))
    block(4, 2424, 2424)
    block(5, 2601, 3110, snp=2700)
    block(1, 2601, 3110, mapq=0)
    block(2, 3111, 3111)
    block(5, 3113, 3500, snp=3300)
    block(5, 3701, 4098, snp=3800)
    block(1, 3701, 4150)
    reads.sort(key=lambda r: r["pos"])
    bam = str(directory / "in.bam")
    bu.write_bam(bam, [("ctg", CONTIG_LEN)], {0: reads}, flush_every=7)
    return dict(bam=bam, ref=ref, reads=reads)


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    return build_job(tmp_path_factory.mktemp("coverage_abi"))


def _depths(job, windows):
    """depth_numpy of every window (start, end inclusive) over the reads its region's fetch takes: those of REGIONS[r] = [a, b]
    with pos < b and a base behind a, mapping quality >= 1."""
    return [depth_numpy([r for r in job["reads"] if r["pos"] < fb and r["pos"] + bu.ref_length(r["cigar"]) > fa], a, b,
                        MIN_SNP_Q, MIN_INDEL_Q, 1) for (a, b), (fa, fb) in zip(windows, REGIONS)]


def _expected(job, windows, bins=BINS, table=None):
    """-> ([(region, start, end, bin)], bases [n, 8], sums [n]) by the numpy rule."""
    runs, bases, sums = [], [], []
    for r, ((a, b), depth) in enumerate(zip(windows, _depths(job, windows))):
        on = None if table is None else Targets.contains(table[0], table[1], np.arange(a, b + 1, dtype=np.int64))
        s, e, k = Coverage.runs_numpy(depth, a, bins, on)
        runs += [(r, x, y, z) for x, y, z in zip(s.tolist(), e.tolist(), k.tolist())]
        t = Coverage.totals_numpy(depth, bins, on)
        bases.append(t[0])
        sums.append(t[1])
    return runs, np.array(bases, np.int64), np.array(sums, np.int64)


def _concat(outs):
    return dict(candidates=[c for o in outs for c in o["candidates"]], per_region=[len(o["positions"]) for o in outs],
                **{k: np.concatenate([o[k] for o in outs]) for k in KEYS})


def _equal(got, want):
    assert got["per_region"] == want["per_region"]
    assert got["candidates"] == want["candidates"]
    for key in KEYS:
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key


class HostForm(object):
    """pa_encoder_generate_summary_batch over reads the host clipped (BAM_handler.get_reads), on this thread's handle."""

    def __init__(self, job):
        from pepper_amd.variant.bam import BAM_handler
        from pepper_amd.variant import PEPPER_VARIANT as pv
        handler = BAM_handler(job["bam"])
        self.flats = [handler.get_reads("ctg", a, b, False, 1, 1).as_pileup() for a, b in REGIONS]
        self.gens = [pv.RegionalSummaryGenerator("ctg", a, b, job["ref"][a - OFF:b + 1 - OFF]) for a, b in REGIONS]
        self.pv = pv
        self.lib, self.enc = pv._encoder(0)

    def set_device_candidates(self, on):
        self.pv.set_device_candidates(on)

    def candidate_calls(self):
        return self.pv.candidate_calls()

    def run(self, windows=None):
        return _concat(self.pv.generate_summary_arrays_batch(self.gens, self.flats, *PARAMS, list(windows or REGIONS), 32, 26, False))

    def close(self):
        self.lib.pa_encoder_set_depth_bins(self.enc, 0, None)
        self.pv._send_targets(self.lib, self.enc, None)
        self.pv.set_device_candidates(False)


class PackedForm(object):
    """pa_encoder_stage_packed + pa_encoder_run_staged over the reads as the BAM stores them, on a handle of its own."""

    def __init__(self, job, sampling=None):
        from pepper_amd.variant.bam import BAM_handler
        from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
        self.packed = PackedEncoder(0, arena_bytes=16 << 20)
        self.lib, self.enc = self.packed.lib, self.packed.enc
        n_done, self.region_pairs, self.counts = self.packed.pack(BAM_handler(job["bam"]), "ctg", [a for a, _ in REGIONS],
                                                                  [b for _, b in REGIONS], False, 1)
        assert n_done == len(REGIONS)
        self.refs = [job["ref"][a - OFF:b + 1 - OFF] for a, b in REGIONS]

    def set_device_candidates(self, on):
        self.packed.set_device_candidates(on)

    def candidate_calls(self):
        return self.packed.candidate_calls()

    def run(self, windows=None):
        outs, live = self.packed.encode(list(REGIONS), self.refs, self.region_pairs, self.counts, PARAMS, list(windows or REGIONS))
        assert live[0] == 0 and live[1:].min() > 0                   # the 300-row region has no read
        return _concat(outs)

    def run_again(self):
        self.packed.last.run()
        return _concat(self.packed.last.results())

    def close(self):
        self.packed.close()


def _set_bins(form, bins):
    """pa_encoder_set_depth_bins -> its return code."""
    if bins is None:
        return form.lib.pa_encoder_set_depth_bins(form.enc, 0, None)
    lower = np.ascontiguousarray(bins, np.int32)
    return form.lib.pa_encoder_set_depth_bins(form.enc, len(lower), lower.ctypes.data)


def _set_targets(form, pairs):
    if pairs is None:
        return form.lib.pa_encoder_set_targets(form.enc, 0, None, None)
    starts, ends = np.array([OFF + a for a, _ in pairs], np.int64), np.array([OFF + b for _, b in pairs], np.int64)
    return form.lib.pa_encoder_set_targets(form.enc, len(starts), starts.ctypes.data, ends.ctypes.data)


def _take(form, n_regions=len(REGIONS)):
    """pa_encoder_depth_runs / _totals / _calls / the timing slot of the handle's last run."""
    n = ctypes.c_int64(-1)
    assert form.lib.pa_encoder_depth_runs(form.enc, 0, None, None, None, None, ctypes.byref(n)) == 0
    k = max(1, n.value)
    region, start, end, which = np.zeros(k, np.int32), np.zeros(k, np.int64), np.zeros(k, np.int64), np.zeros(k, np.int32)
    assert form.lib.pa_encoder_depth_runs(form.enc, k, region.ctypes.data, start.ctypes.data, end.ctypes.data, which.ctypes.data, None) == 0
    bases, sums = np.full((n_regions, 8), -1, np.int64), np.full(n_regions, -1, np.int64)
    assert form.lib.pa_encoder_depth_totals(form.enc, n_regions, bases.ctypes.data, sums.ctypes.data) == 0
    runs = list(zip(region[:n.value].tolist(), start[:n.value].tolist(), end[:n.value].tolist(), which[:n.value].tolist()))
    return runs, bases, sums


def _calls(form):
    made, overflows = ctypes.c_int64(), ctypes.c_int64()
    assert form.lib.pa_encoder_depth_calls(form.enc, ctypes.byref(made), ctypes.byref(overflows)) == 0
    return made.value, overflows.value


def _timing(form):
    ms = np.zeros(14, np.float64)
    assert form.lib.pa_encoder_last_timing(form.enc, ms.ctypes.data, 14) == 0
    return ms


def _check(job, form, windows=REGIONS, bins=BINS, table=None):
    want_runs, want_bases, want_sums = _expected(job, windows, bins, table)
    runs, bases, sums = _take(form)
    assert len(runs) == len(want_runs)
    assert runs == want_runs
    assert np.array_equal(bases, want_bases) and np.array_equal(sums, want_sums)
    return runs


@pytest.fixture(scope="module")
def forms(job):
    made = {"host": HostForm(job), "packed": PackedForm(job)}
    yield made
    for form in made.values():
        form.close()


@pytest.fixture(scope="module")
def plain(job, forms):
    """Each form's run on a handle that never had bins: the yardstick of `nothing else changes`."""
    full = {name: form.run() for name, form in forms.items()}
    for name, out in full.items():
        found = set(zip(out["positions"].tolist(), [c[0] for c in out["candidates"]]))
        for p in SNPS:
            assert (OFF + p, "1") in found, (name, p)
        assert out["per_region"][0] == 0 and min(out["per_region"][1:]) > 0
        assert _timing(forms[name])[13] == 0.0
        n = ctypes.c_int64()
        from pepper_amd import _lib
        assert forms[name].lib.pa_encoder_depth_runs(forms[name].enc, 0, None, None, None, None, ctypes.byref(n)) == _lib.PA_ERR_INVALID
    return full


def test_the_layout_is_what_the_docstring_says(job):
    """The expectation itself: heads on rows 0, 1, 511, 512, 513 and the last row of the 1 500-row region, a run per row over the
    (1M1D) read, a stretch of depth 0, a head on the last row of the 513-row window, one run for the region without reads."""
    runs, bases, sums = _expected(job, REGIONS)
    by_region = [[(s - REGIONS[r][0], e - REGIONS[r][0], b) for q, s, e, b in runs if q == r] for r in range(4)]
    assert by_region[0] == [(0, 300, 0)]
    assert by_region[3] == [(0, 1, 0), (1, 511, 2), (511, 512, 1), (512, 513, 0), (513, 901, 2), (901, 1101, 0), (1101, 1499, 2), (1499, 1500, 1)]
    assert by_region[2][-1] == (512, 513, 1) and by_region[2][-2] == (388, 512, 2)
    comb = [(s, e, b) for s, e, b in by_region[1] if 202 <= s < 301]      # (row 201 has the depth of the rows in front of it)
    assert len(comb) == 99 and all(e - s == 1 for s, e, _ in comb) and [b for _, _, b in comb] == [1, 2] * 49 + [1]
    assert (301, 400, 0) in by_region[1]
    # the rescued anchor counts, the other base of quality 0 does not
    depth = _depths(job, REGIONS)[1]
    assert depth[50] == 3 and depth[60] == 2 and depth[49] == 3
    assert bases[0].tolist() == [300, 0, 0, 0, 0, 0, 0, 0] and sums[0] == 0 and sums[3] == 5 * (510 + 388 + 398) + 399 + 2


@pytest.mark.parametrize("device_candidates", [False, True])
@pytest.mark.parametrize("name", ["host", "packed"])
def test_runs_ends_bins_and_totals(job, forms, plain, name, device_candidates):
    form = forms[name]
    form.set_device_candidates(device_candidates)
    try:
        before, calls_before = form.candidate_calls(), _calls(form)
        assert _set_bins(form, BINS) == 0
        got = form.run()
        runs = _check(job, form)
        assert len(runs) >= 100
        after = form.candidate_calls()
        assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if device_candidates else (0, 0))
        assert _calls(form) == (calls_before[0] + 1, calls_before[1])            # one more run with bins, no overflow
        assert _timing(form)[13] > 0.0
        _equal(got, plain[name])                                                  # candidates and images do not depend on the bins
        # a buffer too small is refused, not filled in part
        from pepper_amd import _lib
        short = np.zeros(4, np.int64)
        assert form.lib.pa_encoder_depth_runs(form.enc, 4, None, short.ctypes.data, None, None, None) == _lib.PA_ERR_INVALID
        # other bins: mosdepth-style, eight of them
        eight = [0, 1, 2, 3, 4, 5, 6, 1000]
        assert _set_bins(form, eight) == 0
        _equal(form.run(), plain[name])
        _check(job, form, bins=eight)
        assert _set_bins(form, [0]) == 0
        form.run()
        assert [(r, e - s, b) for r, s, e, b in _check(job, form, bins=[0])] == [(0, 300, 0), (1, 512, 0), (2, 513, 0), (3, 1500, 0)]
        # bins off again: byte for byte the run of the handle that never had them, and no runs to fetch
        assert _set_bins(form, None) == 0
        _equal(form.run(), plain[name])
        assert _timing(form)[13] == 0.0
        assert form.lib.pa_encoder_depth_runs(form.enc, 0, None, None, None, None, None) == _lib.PA_ERR_INVALID
    finally:
        _set_bins(form, None)
        form.set_device_candidates(False)


def test_run_staged_twice(job, forms, plain):
    form = forms["packed"]
    try:
        assert _set_bins(form, BINS) == 0
        form.run()
        first = _check(job, form)
        _equal(form.run_again(), plain["packed"])
        assert _check(job, form) == first
        assert _set_bins(form, [0, 2]) == 0                           # holds for a batch staged before it was set
        form.run_again()
        _check(job, form, bins=[0, 2])
    finally:
        _set_bins(form, None)


@pytest.mark.parametrize("name", ["host", "packed"])
def test_a_window_narrower_than_the_region(job, forms, name):
    """Rows outside [candidate_region_start, candidate_region_end] are not reported; a window that reaches over the region is cut."""
    form = forms[name]
    (a0, b0), (a1, b1), (a2, b2), (a3, b3) = REGIONS
    windows = [(a0 + 37, b0 - 41), (a1 + 201, a1 + 300), (a2 - 50, b2 + 50), (a3 + 511, b3 + 9)]
    cut = [(a0 + 37, b0 - 41), (a1 + 201, a1 + 300), (a2, b2), (a3 + 511, b3)]
    try:
        assert _set_bins(form, BINS) == 0
        form.run(windows)
        runs = _check(job, form, windows=cut)
        assert [r for r in runs if r[0] == 1][0][1:3] == (a1 + 201, a1 + 202) and len([r for r in runs if r[0] == 1]) == 100
        assert [r for r in runs if r[0] == 3][0][1] == a3 + 511
    finally:
        _set_bins(form, None)


@pytest.mark.parametrize("name", ["host", "packed"])
def test_with_targets(job, forms, name):
    form = forms[name]
    table = (np.array([OFF + a for a, _ in TARGETS], np.int64), np.array([OFF + b for _, b in TARGETS], np.int64))
    try:
        assert _set_targets(form, TARGETS) == 0
        without_bins = form.run()
        assert sum(without_bins["per_region"]) >= 2                    # 1500 and 3800 are targets; 1850, 2700 and 3300 are not
        assert _set_bins(form, BINS) == 0
        _equal(form.run(), without_bins)
        runs = _check(job, form, table=table)
        assert [(r, s - OFF, e - OFF, b) for r, s, e, b in runs if r == 0] == [(0, 1000, 1300, -1)]
        edges = {(s - OFF, e - OFF) for r, s, e, b in runs if b == -1}
        assert (1913, 2415) in edges and (3112, 3113) in edges and (2610, 3100) in edges and (3501, 3600) in edges
        _runs, bases, _sums = _take(form)
        assert bases[0].sum() == 0 and bases[2].sum() == 1 + 10 and bases[3].sum() == 10 + 12 + 17 + 1 + 300
        assert _set_targets(form, None) == 0                            # the table gone, the bins still set
        form.run()
        _check(job, form)
    finally:
        _set_bins(form, None)
        _set_targets(form, None)


REFUSED = {"nine bins": (list(range(9)), "entry 8"), "first bound not 0": ([1, 2, 3], "entry 0"), "equal bounds": ([0, 3, 3], "entry 2"),
           "descending": ([0, 5, 2], "entry 2"), "negative": ([0, -4], "entry 1")}


@pytest.mark.parametrize("name", ["host", "packed"])
def test_refused_bins_leave_the_previous_bins(job, forms, name):
    from pepper_amd import _lib
    form = forms[name]
    try:
        assert _set_bins(form, [0, 2, 4]) == 0
        for why, (bins, entry) in REFUSED.items():
            assert _set_bins(form, bins) == _lib.PA_ERR_INVALID, why
            assert entry in form.lib.pa_last_error().decode(), (why, form.lib.pa_last_error().decode())
        assert form.lib.pa_encoder_set_depth_bins(form.enc, -1, None) == _lib.PA_ERR_INVALID
        assert form.lib.pa_encoder_set_depth_bins(form.enc, 2, None) == _lib.PA_ERR_INVALID
        form.run()
        _check(job, form, bins=[0, 2, 4])
        # ... and refused on a handle without bins: still without
        assert _set_bins(form, None) == 0
        assert _set_bins(form, REFUSED["descending"][0]) == _lib.PA_ERR_INVALID
        form.run()
        assert form.lib.pa_encoder_depth_runs(form.enc, 0, None, None, None, None, None) == _lib.PA_ERR_INVALID
    finally:
        _set_bins(form, None)


def test_a_run_that_overflows_its_buffer_is_exact_and_counted(job, plain, monkeypatch):
    """PEPPER_AMD_DEPTH_RUN_CAP (read by pa_encoder_set_depth_bins) gives the run records room for 16 runs; the batch has more
    than 100: the second emit into a buffer of the scanned total gives the same answer, and the counter says so."""
    monkeypatch.setenv("PEPPER_AMD_DEPTH_RUN_CAP", "16")
    form = PackedForm(job)
    try:
        assert _calls(form) == (0, 0)
        assert _set_bins(form, BINS) == 0
        _equal(form.run(), plain["packed"])
        assert len(_check(job, form)) >= 100
        assert _calls(form) == (1, 1)
        form.run_again()                                              # the buffer has grown: no second overflow
        _check(job, form)
        assert _calls(form) == (2, 1)
    finally:
        form.close()


def test_a_pooled_handle_does_not_carry_bins_over(job):
    from pepper_amd import _lib
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    enc = PackedEncoder.acquire(0, 16 << 20)
    enc.set_depth_bins(BINS)
    enc.release()
    others = []
    again = PackedEncoder.acquire(0, 16 << 20)
    while again is not enc:
        others.append(again)
        assert len(others) < 64
        again = PackedEncoder.acquire(0, 16 << 20)
    for other in others:
        other.release()
    try:
        form = PackedForm.__new__(PackedForm)
        form.packed, form.lib, form.enc = again, again.lib, again.enc
        from pepper_amd.variant.bam import BAM_handler
        n_done, form.region_pairs, form.counts = again.pack(BAM_handler(job["bam"]), "ctg", [a for a, _ in REGIONS], [b for _, b in REGIONS], False, 1)
        form.refs = [job["ref"][a - OFF:b + 1 - OFF] for a, b in REGIONS]
        form.run()
        with pytest.raises(_lib.PepperAmdError):
            again.depth_runs()
        again.set_depth_bins(BINS)
        form.run()
        region, start, end, which = again.depth_runs()
        want = _expected(job, REGIONS)[0]
        assert list(zip(region.tolist(), start.tolist(), end.tolist(), which.tolist())) == want
        assert again.depth_calls() == (1, 0)
    finally:
        again.close()


# ---- the reservoir sample ---------------------------------------------------------------------------------------------------
def test_runs_after_the_device_sample_are_those_of_the_kept_reads(tmp_path):
    """~60x of short reads over one region of 700 positions, sampled down to 40 reads on the device: the depths are those of the
    reads pa_encoder_pair_live reports kept."""
    from pepper_amd.variant.bam import BAM_handler
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    rng = np.random.default_rng(515)
    start, length = 20_000, 700
    ref = pu.random_reference(rng, length)
    reads = [r for r in pu.simulate_reads(rng, ref, start, n_reads=60 * length // 150, read_len=(100, 200), mapq_zero_rate=0.0, clip_rate=0.2)
             if not any(op in (3, 6) for op, _ in r["cigar"])]
    for i, r in enumerate(reads):
        r["name"] = "read_%05d" % i
    bam = str(tmp_path / "deep.bam")
    bu.write_bam(bam, [("ctg", 50_000)], {0: reads}, flush_every=31)
    enc = PackedEncoder(0, arena_bytes=16 << 20)
    try:
        window = (start, start + length - 1)
        n_done, region_pairs, counts = enc.pack(BAM_handler(bam), "ctg", [window[0]], [window[1]], False, 1)
        assert n_done == 1 and counts[1] > 200
        # the packed reads are a subsequence of the reads as written: matched by position, bases and operations
        table, at, mine = enc.reads[:counts[0]], 0, []
        for rec in table:
            while not (reads[at]["pos"] == rec["pos"] and len(reads[at]["seq"]) == rec["l_seq"] and len(reads[at]["cigar"]) == rec["n_cigar"]):
                at += 1
            mine.append(reads[at])
            at += 1
        enc.set_depth_bins([0, 1, 3, 10, 20])
        outs, live = enc.encode([window], [ref], region_pairs, counts, PARAMS, [window], sampling=(2719747673, 40, 1.0))
        assert live[0] == 40 and enc.sampled() == (1, counts[1] - 40)
        keep = enc.pair_live(counts[1])
        assert keep.sum() == 40
        kept = [mine[enc.pair_read[p]] for p in range(counts[1]) if keep[p]]
        depth = depth_numpy(kept, window[0], window[1], MIN_SNP_Q, MIN_INDEL_Q, 1)
        assert depth.max() >= 10 and depth_numpy(mine, window[0], window[1], MIN_SNP_Q, MIN_INDEL_Q, 1).mean() > 40
        s, e, k = Coverage.runs_numpy(depth, window[0], [0, 1, 3, 10, 20])
        region, start_, end_, which = enc.depth_runs()
        assert len(s) > 5 and region.tolist() == [0] * len(s)
        assert start_.tolist() == s.tolist() and end_.tolist() == e.tolist() and which.tolist() == k.tolist()
        bases, sums = enc.depth_totals(1)
        want = Coverage.totals_numpy(depth, [0, 1, 3, 10, 20])
        assert bases[0].tolist() == want[0].tolist() and sums[0] == want[1]
        assert enc.depth_calls() == (1, 0)
    finally:
        enc.close()
