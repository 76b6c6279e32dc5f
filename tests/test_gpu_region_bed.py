"""pa_encoder_set_targets through the C ABI: candidates only at positions inside a table of half-open intervals.

The yardstick is always the unrestricted run of the same form, filtered on the host by Targets.contains: positions, depths,
frequencies, names and int8 images of the restricted run are the unrestricted run's rows with `contains` true, in order --
windows are gathered from the whole matrix, so a kept candidate's image is the unrestricted one byte for byte.

One batch of four regions of one contig with 300, 512, 513 and 1 500 positions (a partial tile, exactly the positions of one
tile, a second tile with one position, three tiles; each matrix has one more, all-zero, row).  The table has edges on rows 0,
511, 512 and 513 of the 1 500-row region, on the first and last row of the 513-row region, an interval of one base, an
interval over the end of one region and the start of the next, and none inside the 300-row region.  A 50 % SNP sits on
start - 1, start, end - 1 and end of every interval; a 3-base insert is anchored on one end - 1, a 6-base deletion on one
start - 1 (it reaches into the target and is dropped: only the anchor counts) and another on one end - 1 (kept)."""
import ctypes

import numpy as np
import pytest

import bam_utils as bu
import pileup_utils as pu
from pepper_amd.variant import Targets

pytestmark = pytest.mark.gpu

OFF = 350_000                        # the regions lie in the middle of a 700 kb coordinate range (the large table's test)
CONTIG_LEN = 700_000
SPAN = 5000                          # bases of the contig that have reads: OFF .. OFF + SPAN
REGIONS = [(OFF + 1000, OFF + 1299), (OFF + 1400, OFF + 1911), (OFF + 1912, OFF + 2424), (OFF + 2600, OFF + 4099)]
# (start, end) half-open, relative to OFF.  In the 1 500-row region (rows = position - 2600): [2600, 2610) starts on row 0;
# [3100, 3112) has end - 1 on row 511 and end on row 512; [3113, 3130) has start - 1 on row 512 and start on row 513;
# [3500, 3501) is one base.  [1900, 1913) spans the end of the 512-row region and row 0 of the 513-row region, [2415, 2425)
# ends on that region's last row.  Nothing inside 1000 .. 1299; the first and the last interval touch no region at all.
TARGETS = [(900, 950), (1500, 1600), (1900, 1913), (2415, 2425), (2600, 2610), (3100, 3112), (3113, 3130), (3500, 3501),
           (3600, 3900), (4200, 4300)]
INSERT_AT, DELETION_IN_AT, DELETION_OUT_AT = 2609, 1499, 1599      # end - 1 of [2600, 2610); start - 1 and end - 1 of [1500, 1600)
PARAMS = (1, 1, 0.1, 0.15, 0.15, 3, 0.1, 0.12, 2, False)
KEYS = ("positions", "depths", "candidate_frequency", "images")


def _table(pairs=TARGETS, off=OFF):
    return (np.array([a + off for a, _ in pairs], np.int64), np.array([b + off for _, b in pairs], np.int64))


def _in_a_region(p):
    return any(a <= p <= b for a, b in REGIONS)


def build_job(directory):
    """-> dict(bam, ref (the SPAN bases at OFF), snps {position: alt}, edge positions in / out of the targets)."""
    assert [b - a + 1 for a, b in REGIONS] == [300, 512, 513, 1500]
    rng = np.random.default_rng(7301)
    ref = pu.random_reference(rng, SPAN)

    def alt(p):
        return "ACGT"[("ACGT".index(ref[p]) + 1 + p % 3) % 4]
    edges_in, edges_out = set(), set()
    for s, e in TARGETS:
        edges_in.update((s, e - 1))
        edges_out.update((s - 1, e))
    edges_out -= edges_in                                          # (of a one-base interval start == end - 1)
    assert not any(Targets.contains(*_table(), [OFF + p for p in edges_out]).tolist())
    background = rng.choice(np.arange(1000, 4100), 420, replace=False).tolist()
    snps = {OFF + p: (alt(p), 0.5) for p in sorted(edges_in | edges_out | set(background))}
    indels = {OFF + INSERT_AT: ("I", "GAT", 0.5), OFF + DELETION_IN_AT: ("D", 6, 0.5), OFF + DELETION_OUT_AT: ("D", 6, 0.5)}
    reads = pu.simulate_reads(rng, ref, OFF, n_reads=30 * SPAN // 400, read_len=(200, 600), snp_sites=snps, indel_sites=indels,
                              clip_rate=0.2, mapq_zero_rate=0.0)
    reads = sorted([r for r in reads if not any(op in (3, 6) for op, _ in r["cigar"])], key=lambda r: r["pos"])
    for i, r in enumerate(reads):
        r["name"] = "read_%05d" % i
    bam = str(directory / "in.bam")
    bu.write_bam(bam, [("ctg", CONTIG_LEN)], {0: reads}, flush_every=37)
    return dict(bam=bam, ref=ref, snps={p: a for p, (a, _) in snps.items()},
                edges_in=sorted(OFF + p for p in edges_in if _in_a_region(OFF + p)),
                edges_out=sorted(OFF + p for p in edges_out if _in_a_region(OFF + p)))


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    return build_job(tmp_path_factory.mktemp("region_bed_abi"))


def _concat(outs):
    """The regions' results back to back, names as a list."""
    return dict(candidates=[c for o in outs for c in o["candidates"]], per_region=[len(o["positions"]) for o in outs],
                **{k: np.concatenate([o[k] for o in outs]) for k in KEYS})


def _filtered(full, table):
    keep = Targets.contains(table[0], table[1], full["positions"])
    at, per_region = 0, []
    for n in full["per_region"]:
        per_region.append(int(keep[at:at + n].sum()))
        at += n
    return dict(candidates=[c for c, k in zip(full["candidates"], keep) if k], per_region=per_region,
                **{k: full[k][keep] for k in KEYS})


def _equal(got, want):
    assert got["per_region"] == want["per_region"]
    assert got["candidates"] == want["candidates"]
    for key in KEYS:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key


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

    def run(self):
        return _concat(self.pv.generate_summary_arrays_batch(self.gens, self.flats, *PARAMS, list(REGIONS), 32, 26, False))

    def close(self):
        self.pv._send_targets(self.lib, self.enc, None)
        self.pv.set_device_candidates(False)


class PackedForm(object):
    """pa_encoder_stage_packed + pa_encoder_run_staged over the reads as the BAM stores them, on a handle of its own."""

    def __init__(self, job):
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

    def run(self):
        outs, live = self.packed.encode(list(REGIONS), self.refs, self.region_pairs, self.counts, PARAMS, list(REGIONS))
        assert live.min() > 0
        return _concat(outs)

    def run_again(self):
        """pa_encoder_run_staged once more on the batch the last run() staged."""
        self.packed.last.run()
        return _concat(self.packed.last.results())

    def close(self):
        self.packed.close()


def _set(form, table):
    """pa_encoder_set_targets -> its return code (the table: (starts, ends) or None)."""
    if table is None:
        return form.lib.pa_encoder_set_targets(form.enc, 0, None, None)
    starts, ends = np.ascontiguousarray(table[0], np.int64), np.ascontiguousarray(table[1], np.int64)
    return form.lib.pa_encoder_set_targets(form.enc, len(starts), starts.ctypes.data, ends.ctypes.data)


@pytest.fixture(scope="module")
def forms(job):
    made = {"host": HostForm(job), "packed": PackedForm(job)}
    yield made
    for form in made.values():
        form.close()


@pytest.fixture(scope="module")
def unrestricted(job, forms):
    """The yardstick of each form, computed once: its run without a table, and that this comparison is not vacuous."""
    full = {name: form.run() for name, form in forms.items()}
    table = _table()
    for name, out in full.items():
        found = set(zip(out["positions"].tolist(), out["candidates"]))
        for p in job["edges_in"] + job["edges_out"]:
            assert (p, "1" + job["snps"][p]) in found, (name, p - OFF)
        at = {p: [c for q, c in found if q == OFF + p] for p in (INSERT_AT, DELETION_IN_AT, DELETION_OUT_AT)}
        assert any(c[0] == "2" and len(c) == 5 for c in at[INSERT_AT]), name
        assert any(c[0] == "3" and len(c) == 8 for c in at[DELETION_IN_AT]) and any(c[0] == "3" and len(c) == 8 for c in at[DELETION_OUT_AT]), name
        inside = Targets.contains(table[0], table[1], out["positions"])
        assert inside.sum() >= 40 and (~inside).sum() >= 40, (name, int(inside.sum()), int((~inside).sum()))
        assert out["per_region"][0] > 0                     # the 300-row region has candidates to lose
    return full


def _check_restricted(job, got, full, table=None):
    table = _table() if table is None else table
    _equal(got, _filtered(full, table))
    return got


@pytest.mark.parametrize("device_candidates", [False, True])
@pytest.mark.parametrize("name", ["host", "packed"])
def test_restricted_run_is_the_unrestricted_run_filtered(job, forms, unrestricted, name, device_candidates):
    form, full = forms[name], unrestricted[name]
    form.set_device_candidates(device_candidates)
    try:
        before = form.candidate_calls()
        assert _set(form, _table()) == 0
        got = _check_restricted(job, form.run(), full)
        after = form.candidate_calls()
        # with the device enumeration on, the call was enumerated there (off: neither counter moves)
        assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if device_candidates else (0, 0))
        assert got["per_region"][0] == 0 and sum(got["per_region"]) >= 40
        found = set(zip(got["positions"].tolist(), got["candidates"]))
        for p in job["edges_in"]:
            assert (p, "1" + job["snps"][p]) in found, p - OFF
        for p in job["edges_out"]:
            assert not any(q == p for q, _ in found), p - OFF
        at = {p: [c for q, c in found if q == OFF + p] for p in (INSERT_AT, DELETION_IN_AT, DELETION_OUT_AT)}
        assert any(c[0] == "2" and len(c) == 5 for c in at[INSERT_AT])            # anchored on end - 1: kept
        assert at[DELETION_IN_AT] == []                                            # anchored on start - 1, reaching in: dropped
        assert any(c[0] == "3" and len(c) == 8 for c in at[DELETION_OUT_AT])      # anchored on end - 1, reaching out: kept
        # no table again: the unrestricted result byte for byte
        assert _set(form, None) == 0
        _equal(form.run(), full)
    finally:
        _set(form, None)
        form.set_device_candidates(False)


def test_run_staged_twice_and_a_second_table(job, forms, unrestricted):
    form, full = forms["packed"], unrestricted["packed"]
    try:
        assert _set(form, _table()) == 0
        first = _check_restricted(job, form.run(), full)
        _equal(form.run_again(), first)
        _equal(form.run_again(), first)
        # a second table replaces the first (and holds for a batch staged before it was set: the verdicts are written per run)
        other = _table([(1000, 1100), (1250, 2000), (4000, 4099)])
        assert _set(form, other) == 0
        got = _check_restricted(job, form.run_again(), full, other)
        assert got["per_region"][0] > 0 and got["per_region"] != first["per_region"]
        _check_restricted(job, form.run(), full, other)
    finally:
        _set(form, None)


REFUSED = {
    "descending": [(2000, 2100), (1500, 1600)],
    "overlapping": [(1500, 1600), (1599, 1700)],
    "touching": [(1500, 1600), (1600, 1700)],
    "start == end": [(1500, 1600), (1700, 1700)],
    "negative start": [(-OFF - 5, -OFF + 10), (1500, 1600)],
}


@pytest.mark.parametrize("name", ["host", "packed"])
def test_refused_tables_leave_the_previous_table(job, forms, unrestricted, name):
    from pepper_amd import _lib
    form, full = forms[name], unrestricted[name]
    try:
        assert _set(form, _table()) == 0
        for why, pairs in REFUSED.items():
            assert _set(form, _table(pairs)) == _lib.PA_ERR_INVALID, why
            message = form.lib.pa_last_error().decode()
            assert "interval %d" % (0 if why == "negative start" else 1) in message, (why, message)
        assert form.lib.pa_encoder_set_targets(form.enc, -1, None, None) == _lib.PA_ERR_INVALID
        assert form.lib.pa_encoder_set_targets(form.enc, 2, None, None) == _lib.PA_ERR_INVALID
        _check_restricted(job, form.run(), full)
        # ... and refused on a handle without a table: still without one
        assert _set(form, None) == 0
        assert _set(form, _table(REFUSED["touching"])) == _lib.PA_ERR_INVALID
        _equal(form.run(), full)
    finally:
        _set(form, None)


@pytest.mark.parametrize("name", ["host", "packed"])
def test_a_table_of_100000_one_base_intervals(job, forms, unrestricted, name):
    """Every 7th position of the 700 kb range, the regions in its middle: the workgroup's binary search over the whole table,
    then ~73 intervals per tile."""
    form, full = forms[name], unrestricted[name]
    starts = np.arange(0, CONTIG_LEN, 7, dtype=np.int64)
    assert len(starts) == 100_000
    table = (starts, starts + 1)
    inside = Targets.contains(table[0], table[1], full["positions"])
    assert inside.sum() >= 20 and (~inside).sum() >= 100
    try:
        assert _set(form, table) == 0
        _check_restricted(job, form.run(), full, table)
    finally:
        _set(form, None)


def test_a_pooled_handle_does_not_carry_targets_over(job, unrestricted):
    """PackedEncoder.acquire hands out what release() returned: without the last user's targets."""
    from pepper_amd.variant.bam import BAM_handler
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    enc = PackedEncoder.acquire(0, 16 << 20)
    table = _table()
    enc.set_targets(table, "ctg")
    handler = BAM_handler(job["bam"])
    refs = [job["ref"][a - OFF:b + 1 - OFF] for a, b in REGIONS]

    def run(e):
        n_done, region_pairs, counts = e.pack(handler, "ctg", [a for a, _ in REGIONS], [b for _, b in REGIONS], False, 1)
        assert n_done == len(REGIONS)
        return _concat(e.encode(list(REGIONS), refs, region_pairs, counts, PARAMS, list(REGIONS))[0])
    _equal(run(enc), _filtered(unrestricted["packed"], table))
    enc.release()
    others = []                                         # (idle handles of earlier tests that fit the same request)
    again = PackedEncoder.acquire(0, 16 << 20)
    while again is not enc:
        others.append(again)
        assert len(others) < 64
        again = PackedEncoder.acquire(0, 16 << 20)
    for other in others:
        other.release()
    try:
        _equal(run(again), unrestricted["packed"])
        again.set_targets(table, "ctg")                 # the same contig as before the release: sent again all the same
        _equal(run(again), _filtered(unrestricted["packed"], table))
    finally:
        again.close()
