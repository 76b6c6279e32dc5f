"""pa_encoder_set_ref_confidence through the C ABI: the reference blocks of a run's positions, with their minima.

Every expected value is RefConfidence.gq_numpy / blocks_numpy over refconf_cases.evidence_numpy of the reads the BAM was
written from; none comes from the code under test.  The device reports a run that crosses a tile border as one record per
tile; what is compared is RefConfidence.merge_blocks of its records (the merge has CPU tests of its own).

One batch of four regions of one contig with 300, 512, 513 and 1 500 positions, the regions and the two forms of
tests/test_gpu_coverage.py.  The reads are laid out by hand (positions relative to OFF):
  1000 - 1299   no read at all: one block of GQ 0, MIN_DP 0
  1400 - 1500   three all-reference reads: GQ 9; two of them carry a SNP on 1420 (a candidate, GQ 0); the reference has an N on
                1450: GQ 0 whatever the reads say
  1520 - 1560   three reads, one of which opens an insert behind 1540: n_ref 2, n_alt 1 on the anchor
  1601 - 1700   two reads and one read of (1M1D) x 50: (3, 0) and (2, 1) alternate with every base -- a block per row
  1950 - 2200   twenty all-reference reads: GQ 50; one of them mismatches on 2100, below the SNP threshold: a one-row block of
                GQ 30 and no candidate
  2230 - 2280   130 identical reads, past the int8 clamp of 125 and past the rescale: MIN_DP 130, GQ 50
  2300 - 2424   twenty reads that go on to 2450: a block that ends on the last row of the 513-row window, row 0 of its second tile
  3000 - 3300   eighteen reads, and two more over 3000 - 3111: rows 400 - 700 of the 1 500-row region, one block over rows 511 /
                512 / 513 whose smallest depth, 18, lies in the second tile; two of the reads carry a SNP on 3250
  3701 - 3800   five reads of mapping quality 0: they do not count, GQ 0 and MIN_DP 0"""
import ctypes

import numpy as np
import pytest

import bam_utils as bu
import pileup_utils as pu
import test_gpu_coverage as cov
from refconf_cases import evidence_numpy
from pepper_amd.variant import Coverage, RefConfidence, Targets

pytestmark = pytest.mark.gpu

OFF, REGIONS, TARGETS = cov.OFF, cov.REGIONS, cov.TARGETS
BANDS = list(RefConfidence.DEFAULT_BANDS)
TABLE = RefConfidence.build_table()
SNPS = (1420, 3250)
N_AT = 1450


def build_job(directory):
    ref = pu.random_reference(np.random.default_rng(9107), cov.SPAN)
    ref = ref[:N_AT] + "N" + ref[N_AT + 1:]
    M, I, D = pu.OP_M, pu.OP_I, pu.OP_D
    reads = []

    def block(k, lo, hi, snp=None, **kw):
        for j in range(k):
            reads.append(cov._read(ref, lo, [(M, hi - lo + 1)], "b%d_%d" % (lo, j), alts=(snp,) if snp is not None and j < 2 else (),
                                   reverse=j % 2 == 1, **kw))
    block(3, 1400, 1500, snp=1420)
    block(2, 1520, 1560)
    reads.append(cov._read(ref, 1520, [(M, 21), (I, 2), (M, 20)], "insert"))
    block(2, 1601, 1700)
    reads.append(cov._read(ref, 1601, [(M, 1), (D, 1)] * 50, "comb"))
    block(19, 1950, 2200)
    reads.append(cov._read(ref, 1950, [(M, 251)], "lone", alts=(2100,)))
    block(130, 2230, 2280)
    block(20, 2300, 2450)
    block(18, 3000, 3300, snp=3250)
    block(2, 3000, 3111)
    block(5, 3701, 3800, mapq=0)
    reads.sort(key=lambda r: r["pos"])
    bam = str(directory / "in.bam")
    bu.write_bam(bam, [("ctg", cov.CONTIG_LEN)], {0: reads}, flush_every=7)
    return dict(bam=bam, ref=ref, reads=reads)


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    return build_job(tmp_path_factory.mktemp("refconf_abi"))


def _evidence(job, windows):
    return [evidence_numpy([r for r in job["reads"] if r["pos"] < fb and r["pos"] + bu.ref_length(r["cigar"]) > fa],
                           job["ref"][a - OFF:b + 1 - OFF], a, b, cov.MIN_SNP_Q, cov.MIN_INDEL_Q, 1)
            for (a, b), (fa, fb) in zip(windows, REGIONS)]


def _expected(job, windows=REGIONS, bands=BANDS, table=TABLE, targets=None):
    """-> [(region, start, end, band, min_dp, min_gq)] by the numpy rule."""
    out = []
    for r, ((a, b), ev) in enumerate(zip(windows, _evidence(job, windows))):
        on = None if targets is None else Targets.contains(targets[0], targets[1], np.arange(a, b + 1, dtype=np.int64))
        cols = RefConfidence.blocks_numpy(ev[0], RefConfidence.gq_numpy(*ev, table), a, bands, on)
        out += [(r,) + rec for rec in zip(*(c.tolist() for c in cols))]
    return out


def _set(form, table, bands, side=None):
    """pa_encoder_set_ref_confidence -> its return code."""
    if bands is None:
        return form.lib.pa_encoder_set_ref_confidence(form.enc, None, 0, 0, None)
    table = np.ascontiguousarray(table, np.uint8)
    lower = np.ascontiguousarray(bands, np.int32)
    return form.lib.pa_encoder_set_ref_confidence(form.enc, table.ctypes.data, table.shape[0] if side is None else side, len(lower),
                                                  lower.ctypes.data)


def _take(form):
    """pa_encoder_ref_blocks of the handle's last run -> (the records as the device wrote them, the merged blocks)."""
    n = ctypes.c_int64(-1)
    assert form.lib.pa_encoder_ref_blocks(form.enc, 0, None, None, None, None, None, None, ctypes.byref(n)) == 0
    k = max(1, n.value)
    cols = [np.zeros(k, t) for t in (np.int32, np.int64, np.int64, np.int32, np.int32, np.int32)]
    assert form.lib.pa_encoder_ref_blocks(form.enc, k, *[c.ctypes.data for c in cols], None) == 0
    cols = [c[:n.value] for c in cols]
    merged = RefConfidence.merge_blocks(*cols)
    return list(zip(*(c.tolist() for c in cols))), list(zip(*(c.tolist() for c in merged)))


def _calls(form):
    made, overflows = ctypes.c_int64(), ctypes.c_int64()
    assert form.lib.pa_encoder_ref_calls(form.enc, ctypes.byref(made), ctypes.byref(overflows)) == 0
    return made.value, overflows.value


def _timing(form):
    ms = np.zeros(15, np.float64)
    assert form.lib.pa_encoder_last_timing(form.enc, ms.ctypes.data, 15) == 0
    return ms


def _no_blocks(form):
    from pepper_amd import _lib
    return form.lib.pa_encoder_ref_blocks(form.enc, 0, None, None, None, None, None, None, None) == _lib.PA_ERR_INVALID


def _check(job, form, **kw):
    want = _expected(job, **kw)
    raw, merged = _take(form)
    assert len(merged) == len(want)
    assert merged == want
    return raw, merged


def _off(form):
    _set(form, None, None)
    form.lib.pa_encoder_set_depth_bins(form.enc, 0, None)
    form.lib.pa_encoder_set_targets(form.enc, 0, None, None)


@pytest.fixture(scope="module")
def forms(job):
    made = {"host": cov.HostForm(job), "packed": cov.PackedForm(job)}
    yield made
    for form in made.values():
        _off(form)
        form.close()


@pytest.fixture(scope="module")
def plain(job, forms):
    """Each form's run on a handle that never had a table: the yardstick of `nothing else changes`."""
    full = {name: form.run() for name, form in forms.items()}
    for name, out in full.items():
        found = set(zip(out["positions"].tolist(), [c[0] for c in out["candidates"]]))
        for p in SNPS:
            assert (OFF + p, "1") in found, (name, p)
        assert OFF + 2100 not in out["positions"].tolist()             # one read in twenty: below the SNP threshold
        assert _timing(forms[name])[14] == 0.0 and _no_blocks(forms[name])
    return full


def test_the_layout_is_what_the_docstring_says(job):
    want = _expected(job)
    by_region = [[(s - OFF, e - OFF, b, dp, gq) for q, s, e, b, dp, gq in want if q == r] for r in range(4)]
    assert by_region[0] == [(1000, 1300, 0, 0, 0)]
    one = by_region[1]
    assert one[:5] == [(1400, 1420, 1, 3, 9), (1420, 1421, 0, 3, 0), (1421, 1450, 1, 3, 9), (1450, 1451, 0, 3, 0), (1451, 1501, 1, 3, 9)]
    assert (1540, 1541, 0, 3, RefConfidence.gq_value(2, 1)) in one and RefConfidence.gq_value(2, 1) == 0
    comb = [rec for rec in one if 1601 <= rec[0] < 1700]               # (row 1700 goes on into the rows without reads behind it)
    assert len(comb) == 99 and all(e - s == 1 for s, e, _b, _dp, _gq in comb)
    assert [(b, dp, gq) for _s, _e, b, dp, gq in comb] == ([(1, 3, 9), (0, 2, 0)] * 50)[:99]
    assert one[-1] == (1700, 1912, 0, 0, 0)
    two = by_region[2]
    assert (1950, 2100, 6, 20, 50) in two and (2100, 2101, 4, 20, 30) in two and (2101, 2201, 6, 20, 50) in two
    assert (2230, 2281, 6, 130, 50) in two                            # unsaturated, and rescaled to (100, 0)
    assert two[-1] == (2300, 2425, 6, 20, 50)                         # ends on the window's last row
    three = by_region[3]
    assert (3000, 3250, 6, 18, 50) in three                           # rows 400 - 649: depth 20 up to row 511, 18 from row 512
    assert three[-1] == (3301, 4100, 0, 0, 0)                         # the reads of mapping quality 0 over 3701 - 3800 do not show


@pytest.mark.parametrize("device_candidates", [False, True])
@pytest.mark.parametrize("name", ["host", "packed"])
def test_blocks_with_their_minima(job, forms, plain, name, device_candidates):
    from pepper_amd import _lib
    form = forms[name]
    form.set_device_candidates(device_candidates)
    try:
        calls_before = _calls(form)
        assert _set(form, TABLE, BANDS) == 0
        got = form.run()
        raw, merged = _check(job, form)
        assert len(merged) >= 100
        # the block over rows 511 / 512 / 513 came as one record per tile, the minimum of the second smaller
        a3 = REGIONS[3][0]
        halves = [rec for rec in raw if rec[0] == 3 and rec[1] <= a3 + 512 <= rec[2] and rec[3] == 6]
        assert [(s - a3, e - a3, dp, gq) for _r, s, e, _b, dp, gq in halves] == [(400, 512, 20, 50), (512, 650, 18, 50)]
        assert _calls(form) == (calls_before[0] + 1, calls_before[1])
        assert _timing(form)[14] > 0.0 and _timing(form)[13] == 0.0
        cov._equal(got, plain[name])                                  # candidates and images do not depend on the table
        short = np.zeros(4, np.int64)
        assert form.lib.pa_encoder_ref_blocks(form.enc, 4, None, short.ctypes.data, None, None, None, None, None) == _lib.PA_ERR_INVALID
        # another error rate and other bands
        other = RefConfidence.build_table(0.01, 40)
        assert not np.array_equal(other, TABLE)
        assert _set(form, other, [0, 5, 25]) == 0
        cov._equal(form.run(), plain[name])
        _check(job, form, table=other, bands=[0, 5, 25])
        # switched off again: byte for byte the run of the handle that never had a table, nothing counted, nothing to fetch
        assert _set(form, None, None) == 0
        calls = _calls(form)
        cov._equal(form.run(), plain[name])
        assert _timing(form)[14] == 0.0 and _calls(form) == calls and _no_blocks(form)
    finally:
        _off(form)
        form.set_device_candidates(False)


def test_the_packed_form_gives_the_blocks_of_the_host_form(job, forms):
    taken = {}
    for name, form in forms.items():
        try:
            assert _set(form, TABLE, BANDS) == 0
            form.run()
            taken[name] = _take(form)
        finally:
            _off(form)
    assert taken["host"] == taken["packed"] and len(taken["host"][0]) > len(taken["host"][1]) >= 100


def test_run_staged_twice(job, forms, plain):
    form = forms["packed"]
    try:
        assert _set(form, TABLE, BANDS) == 0
        form.run()
        first = _check(job, form)
        cov._equal(form.run_again(), plain["packed"])
        assert _check(job, form) == first
        assert _set(form, TABLE, [0, 30]) == 0                        # holds for a batch staged before it was set
        form.run_again()
        _check(job, form, bands=[0, 30])
    finally:
        _off(form)


@pytest.mark.parametrize("name", ["host", "packed"])
def test_with_targets(job, forms, name):
    form = forms[name]
    table = (np.array([OFF + a for a, _ in TARGETS], np.int64), np.array([OFF + b for _, b in TARGETS], np.int64))
    try:
        assert cov._set_targets(form, TARGETS) == 0
        without = form.run()
        assert _set(form, TABLE, BANDS) == 0
        cov._equal(form.run(), without)
        _raw, merged = _check(job, form, targets=table)
        assert [(r, s - OFF, e - OFF, b) for r, s, e, b, _dp, _gq in merged if r == 0] == [(0, 1000, 1300, -1)]
        edges = {(s - OFF, e - OFF) for r, s, e, b, _dp, _gq in merged if b == -1}
        assert (1913, 2415) in edges and (3112, 3113) in edges and (2610, 3100) in edges
        assert cov._set_targets(form, None) == 0                      # the targets gone, the table still set
        form.run()
        _check(job, form)
    finally:
        _off(form)


@pytest.mark.parametrize("name", ["host", "packed"])
def test_with_depth_bins_at_once(job, forms, plain, name):
    """One instance of the tile kernel serves both: the blocks are as alone, the depth runs as alone."""
    form = forms[name]
    try:
        assert cov._set_bins(form, cov.BINS) == 0
        form.run()
        runs_alone = cov._take(form)
        want_runs = []
        for r, ((a, b), ev) in enumerate(zip(REGIONS, _evidence(job, REGIONS))):
            s, e, k = Coverage.runs_numpy(ev[0], a, cov.BINS)
            want_runs += [(r, x, y, z) for x, y, z in zip(s.tolist(), e.tolist(), k.tolist())]
        assert runs_alone[0] == want_runs
        assert _set(form, TABLE, BANDS) == 0
        cov._equal(form.run(), plain[name])
        _check(job, form)
        both = cov._take(form)
        assert both[0] == runs_alone[0] and np.array_equal(both[1], runs_alone[1]) and np.array_equal(both[2], runs_alone[2])
        assert _timing(form)[13] > 0.0 and _timing(form)[14] > 0.0
        assert cov._set_bins(form, None) == 0                         # the bins gone, the table still set
        form.run()
        _check(job, form)
        assert _timing(form)[13] == 0.0
    finally:
        _off(form)


def _broken_tables():
    rising = TABLE.copy()
    rising[5, 7] = rising[5, 6] + 1                                   # one more read against the reference, a higher GQ
    falling = TABLE.copy()
    falling[9, 0] = falling[8, 0] - 1                                 # one more read for it, a lower GQ
    origin = TABLE.copy()
    origin[0, 0] = 1
    return {"rising with n_alt": (rising, BANDS, None, "(5, 7)"), "falling with n_ref": (falling, BANDS, None, "(9, 0)"),
            "origin": (origin, BANDS, None, "(0, 0)"), "side": (TABLE[:100, :100], BANDS, None, "side 100"),
            "nine bands": (TABLE, list(range(9)), None, "band 8"), "first bound not 0": (TABLE, [1, 2], None, "band 0"),
            "equal bounds": (TABLE, [0, 3, 3], None, "band 2"), "descending": (TABLE, [0, 5, 2], None, "band 2"),
            "negative": (TABLE, [0, -4], None, "band 1"), "above a byte": (TABLE, [0, 256], None, "band 1")}


@pytest.mark.parametrize("name", ["host", "packed"])
def test_refused_settings_leave_the_previous_one(job, forms, name):
    from pepper_amd import _lib
    form = forms[name]
    try:
        assert _set(form, TABLE, [0, 9, 30]) == 0
        for why, (table, bands, side, entry) in _broken_tables().items():
            assert _set(form, table, bands, side) == _lib.PA_ERR_INVALID, why
            assert entry in form.lib.pa_last_error().decode(), (why, form.lib.pa_last_error().decode())
        assert form.lib.pa_encoder_set_ref_confidence(form.enc, None, 101, -1, None) == _lib.PA_ERR_INVALID
        assert form.lib.pa_encoder_set_ref_confidence(form.enc, None, 101, 2, None) == _lib.PA_ERR_INVALID
        form.run()
        _check(job, form, bands=[0, 9, 30])
        # ... and refused on a handle without a table: still without
        assert _set(form, None, None) == 0
        assert _set(form, TABLE, [0, 5, 2]) == _lib.PA_ERR_INVALID
        form.run()
        assert _no_blocks(form)
    finally:
        _off(form)


def test_a_run_that_overflows_its_buffer_is_exact_and_counted(job, plain, monkeypatch):
    """PEPPER_AMD_REF_BLOCK_CAP (read by pa_encoder_set_ref_confidence) gives the records room for 16; the batch has more than
    100: the second emit into a buffer of the scanned total gives the same answer, and the counter says so."""
    monkeypatch.setenv("PEPPER_AMD_REF_BLOCK_CAP", "16")
    form = cov.PackedForm(job)
    try:
        assert _calls(form) == (0, 0)
        assert _set(form, TABLE, BANDS) == 0
        cov._equal(form.run(), plain["packed"])
        assert len(_check(job, form)[1]) >= 100
        assert _calls(form) == (1, 1)
        form.run_again()                                              # the buffer has grown: no second overflow
        _check(job, form)
        assert _calls(form) == (2, 1)
    finally:
        form.close()


def test_a_class_that_holds_across_a_tile_border_with_both_tracks_on(tmp_path):
    """One region of 520 rows, three reads over rows 500 - 519, depth bins and a table set for one run: depth 3 (bin 2) and
    GQ 9 (band 1) on both sides of row 512.  Here the two tracks' head rules differ: the depth track looks back across the
    border -- exactly one run over it --, the block track starts a record with every tile -- exactly two, touching on row
    512, of equal band, each with the numpy rule's minima over its own rows."""
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    from pepper_amd.variant.bam import BAM_handler
    a, b = OFF + 1000, OFF + 1519
    ref = pu.random_reference(np.random.default_rng(9108), cov.SPAN)
    reads = [cov._read(ref, 1500, [(pu.OP_M, 20)], "r%d" % j, reverse=j % 2 == 1) for j in range(3)]
    bam = str(tmp_path / "border.bam")
    bu.write_bam(bam, [("ctg", cov.CONTIG_LEN)], {0: reads}, flush_every=7)
    ev = evidence_numpy(reads, ref[1000:1520], a, b, cov.MIN_SNP_Q, cov.MIN_INDEL_Q, 1)
    gq = RefConfidence.gq_numpy(*ev, TABLE)
    want_runs = [(0,) + rec for rec in zip(*(c.tolist() for c in Coverage.runs_numpy(ev[0], a, cov.BINS)))]
    want_blocks = [(0,) + rec for lo, hi in ((0, 512), (512, 520))
                   for rec in zip(*(c.tolist() for c in RefConfidence.blocks_numpy(ev[0][lo:hi], gq[lo:hi], a + lo, BANDS)))]
    assert want_runs == [(0, a, a + 500, 0), (0, a + 500, a + 520, 2)]
    assert want_blocks == [(0, a, a + 500, 0, 0, 0), (0, a + 500, a + 512, 1, 3, 9), (0, a + 512, a + 520, 1, 3, 9)]
    enc = PackedEncoder(0, arena_bytes=16 << 20)
    try:
        n_done, region_pairs, counts = enc.pack(BAM_handler(bam), "ctg", [a], [b], False, 1)
        assert n_done == 1
        enc.set_depth_bins(cov.BINS)
        enc.set_ref_confidence(TABLE, BANDS)
        enc.encode([(a, b)], [ref[1000:1520]], region_pairs, counts, cov.PARAMS, [(a, b)])
        runs = list(zip(*(c.tolist() for c in enc.depth_runs())))
        blocks = list(zip(*(c.tolist() for c in enc.ref_blocks())))
    finally:
        enc.close()
    assert runs == want_runs
    assert blocks == want_blocks


def test_a_pooled_handle_does_not_carry_the_table_over(job):
    from pepper_amd import _lib
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    enc = PackedEncoder.acquire(0, 16 << 20)
    enc.set_ref_confidence(TABLE, BANDS)
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
        form = cov.PackedForm.__new__(cov.PackedForm)
        form.packed, form.lib, form.enc = again, again.lib, again.enc
        from pepper_amd.variant.bam import BAM_handler
        n_done, form.region_pairs, form.counts = again.pack(BAM_handler(job["bam"]), "ctg", [a for a, _ in REGIONS], [b for _, b in REGIONS], False, 1)
        form.refs = [job["ref"][a - OFF:b + 1 - OFF] for a, b in REGIONS]
        form.run()
        with pytest.raises(_lib.PepperAmdError):
            again.ref_blocks()
        again.set_ref_confidence(TABLE, BANDS)
        form.run()
        merged = RefConfidence.merge_blocks(*again.ref_blocks())
        assert list(zip(*(c.tolist() for c in merged))) == _expected(job)
        assert again.ref_calls() == (1, 0) and again.ref_blocks_ms() > 0.0
    finally:
        again.close()
