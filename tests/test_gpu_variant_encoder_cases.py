"""The variant summary encoder's kernels (pepper_amd/csrc/encoder.hip: segment_reads_kernel, the three instances of
tile_count_kernel, unpack_clip_kernel, the candidate enumerations of host and device) on the hand-built pileups of
tests/variant_encoder_cases.py: tile edges and the previous tile's record, anchoring last bases, the three quality sums of an
insert and its rescue, allele keys at 61 characters and past the reference's end, 64-operation passes, the exception queue at
128 / 129, the vote buffer at 512 / 513, the clamp, the first and last 16 rows of a region, 300 regions in one batch.

Every expected value is the restatement's (oracle/pileup_oracle.cpp), which tests/test_variant_encoder_cases_cpu.py pins to the
reference build, to a golden and to rows worked out by hand on exactly these cases -- or, for the two per-position tracks, the
numpy rules of Coverage / RefConfidence over coverage_cases.depth_numpy / refconf_cases.evidence_numpy.  None comes from the code
under test.  Integer work: bit-exact, no tolerances.

Every case runs host-clipped in a call of its own and in batches of its family in two orders, under both candidate enumerations,
with depth bins (the TILE_DEPTH instance) and with a reference-confidence table (TILE_REFCONF) set, and -- every family but
`letters`, whose bases a BAM cannot hold (variant_encoder_cases.PACKED_FAMILIES) -- from a BAM through PackedEncoder.pack + encode,
where unpack_clip_kernel clips the reads: the expectation there is the restatement over bam_utils.restated_get_reads of the same
reads (which alters some cases: see ALTERED_BY_THE_CLIP in the CPU module).  No case of the catalogue is one the device
enumeration refuses by design (more than 1 024 votes or 16 rare letters at a site): the counter of calls handed back to the
host must not move.

Which case guards which branch of the kernels:
    - the anchoring bit of tile_count_kernel (the entry's bit 4 and the `anch` array): every family with an insert or a
      deletion behind a match run, in every form; by_hand / anchoring_last_base states the counters
    - the rescue in front of `avail + 1 <= 61`: by_hand / rescued_anchor and insert_quality / rescue, in every form
    - next_op read across the 64-lane pass: many_operations / op64_insert_on_511 and op64_deletion_from_512, in every form
    - the extra previous-tile record of segment_reads_kernel: tile_edges / leading, in every host-clipped form.  The packed form
      cannot see it: the clip drops an insert in front of the first aligned base."""
import numpy as np
import pytest

import bam_utils as bu
import pileup_utils as pu
import variant_encoder_cases as vc
from coverage_cases import depth_numpy
from refconf_cases import evidence_numpy
from test_gpu_device_candidates import RULES, _on_and_off
from test_gpu_encoder import _check, _gen_and_flat, _product

pytestmark = pytest.mark.gpu

BINS = list(range(8))
BYTE_KEYS = ("positions", "depths", "candidate_frequency", "images", "images_int32")
REFCONF_FAMILIES = ("anchors", "insert_quality")         # where the blocks themselves are compared with the numpy rule
_families, _want = {}, {}


def family(name):
    if name not in _families:
        _families[name] = vc.FAMILIES[name]()
    return _families[name]


def want(fam, name):
    """The restatement's result: computed once per case, never changed."""
    if (fam, name) not in _want:
        case = family(fam)[name]
        out = pu.run_variant(pu.load_restatement(), vc.pileup(case), vc.params(case))
        for key in ("positions", "depths", "candidate_frequency", "images"):
            out[key].flags.writeable = False
        _want[fam, name] = out
    return _want[fam, name]


def rules_of(case):
    q = vc.params(case)
    return tuple(getattr(q, f) for f in RULES)


def groups_of(fam):
    """The family's cases grouped by their thresholds (a batch call takes one set for all of its regions), in catalogue order."""
    groups = {}
    for name, case in family(fam).items():
        groups.setdefault(rules_of(case), []).append(name)
    return list(groups.items())


def run_batch(fam, names, rules):
    from pepper_amd.variant.PEPPER_VARIANT import generate_summary_arrays_batch
    cases = [family(fam)[n] for n in names]
    piles = [vc.pileup(c) for c in cases]
    gens, flats = zip(*[_gen_and_flat(p) for p in piles])
    windows = [(q.candidate_region_start, q.candidate_region_end) for q in map(vc.params, cases)]
    return generate_summary_arrays_batch(list(gens), list(flats), *rules[:9], bool(rules[9]), windows, 32, 26, False, want_int32=True)


def run_family(fam):
    """Every group of the family as one batch -> {name: result}."""
    out = {}
    for rules, names in groups_of(fam):
        out.update(zip(names, run_batch(fam, names, rules)))
    return out


def check_family(fam, got, what=""):
    assert sorted(got) == sorted(family(fam))
    for name, g in got.items():
        try:
            _check(g, want(fam, name))
        except AssertionError as err:
            raise AssertionError("%s / %s %s: %s" % (fam, name, what, err)) from err


def same_bytes(a, b, what):
    assert sorted(a) == sorted(b)
    for name in a:
        assert a[name]["candidates"] == b[name]["candidates"], (what, name)
        for key in BYTE_KEYS:
            assert a[name][key].dtype == b[name][key].dtype and a[name][key].tobytes() == b[name][key].tobytes(), (what, name, key)


@pytest.fixture(scope="module", autouse=True)
def clean_thread_handle():
    """The per-thread handle is shared with every other module: whatever a test of this one set is off again behind it."""
    yield
    from pepper_amd.variant import PEPPER_VARIANT as pv
    lib, enc = pv._encoder(0)
    pv._send_depth_bins(lib, enc, None)
    pv._send_ref_confidence(lib, enc, None, None)
    pv._send_targets(lib, enc, None)
    pv.set_device_candidates(False)


# ---- host-clipped form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", sorted(vc.FAMILIES))
def test_every_case_in_a_call_of_its_own(fam):
    """RegionalSummaryGenerator.generate_summary_arrays(..., want_int32=True): candidates, positions, depths, frequencies, the
    int32 images and their int8 wrap."""
    seen = 0
    for name, case in family(fam).items():
        try:
            _check(_product(vc.pileup(case), vc.params(case)), want(fam, name))
        except AssertionError as err:
            raise AssertionError("%s / %s: %s" % (fam, name, err)) from err
        seen += len(want(fam, name)["candidates"])
    assert seen > 0


@pytest.mark.parametrize("fam", sorted(vc.FAMILIES))
def test_a_family_as_one_batch_in_two_orders(fam):
    """generate_summary_arrays_batch over the family's cases, then over the same cases in reverse on the same handle: the second
    batch does not see the first.  many_regions: 300 regions of 1, 2, 3 and 513 rows in one call -- every matrix on a row that
    is a multiple of 16, every region's sites and votes in its own slice."""
    check_family(fam, run_family(fam), "in order")
    for rules, names in groups_of(fam):
        back = names[::-1]
        for name, g in zip(back, run_batch(fam, back, rules)):
            try:
                _check(g, want(fam, name))
            except AssertionError as err:
                raise AssertionError("%s / %s reversed: %s" % (fam, name, err)) from err
    check_family(fam, run_family(fam), "in order again")


@pytest.mark.parametrize("fam", sorted(vc.FAMILIES))
def test_both_candidate_enumerations(fam):
    """set_device_candidates(False) and (True): equal results, both the restatement's; the counters move on the device's side by
    the calls made and not at all on the host's -- nothing in the catalogue is handed back."""
    on, off = _on_and_off(lambda: run_family(fam), calls=len(groups_of(fam)), on_host=0)
    same_bytes(on, off, fam)
    check_family(fam, on, "device enumeration")


# ---- packed form ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def packed():
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    enc = PackedEncoder(0, arena_bytes=16 << 20)
    yield enc
    enc.close()


def _packed_both_ways(packed, regions, refs, region_pairs, counts, rules, windows, what):
    """encode under the host's and the device's enumeration -> the results of the two (per region), the reads alive per region."""
    got = {}
    for device in (False, True):
        packed.set_device_candidates(device)
        before = packed.candidate_calls()
        try:
            outs, live = packed.encode(regions, refs, region_pairs, counts, rules, windows, want_int32=True)
        finally:
            packed.set_device_candidates(False)
        after = packed.candidate_calls()
        assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if device else (0, 0)), what
        got[device] = (outs, live.tolist())
    assert got[True][1] == got[False][1]
    return got[False][0], got[True][0], got[False][1]


@pytest.mark.parametrize("fam", [f for f in vc.PACKED_FAMILIES if f not in vc.PACKED_AS_ONE_BATCH])
def test_packed_form_equals_the_restatement_over_the_clipped_reads(fam, packed, tmp_path):
    """The reads written with bam_utils.write_bam, packed as the file stores them and clipped on the device: 4-bit bases at odd
    offsets, the anchored bit across a 64-operation pass, reads over both fetch ends, reads that start on the fetch's last
    position (not fetched).  Under both enumerations."""
    from pepper_amd.variant.bam import BAM_handler
    oracle = pu.load_restatement()
    for name, case in family(fam).items():
        a, b, ref = case[0], case[1], case[2]
        reads, q = vc.bam_reads(case), vc.params(case)
        clipped = bu.restated_get_reads(reads, a, b, False, 1)
        exp = pu.run_variant(oracle, pu.FlatPileup(a, b, ref, clipped), q)
        assert len(exp["candidates"]) > 0
        bam = str(tmp_path / ("%s_%s.bam" % (fam, name)))
        bu.write_bam(bam, [("ctg", b + 2000)], {0: reads}, flush_every=5)
        n_done, region_pairs, counts = packed.pack(BAM_handler(bam), "ctg", [a], [b], False, 1)
        assert n_done == 1
        on_host, on_device, live = _packed_both_ways(packed, [(a, b)], [ref], region_pairs, counts, rules_of(case),
                                                     [(q.candidate_region_start, q.candidate_region_end)], (fam, name))
        assert live == [len(clipped)], (fam, name)
        for device, outs in ((False, on_host), (True, on_device)):
            try:
                _check(outs[0], exp)
            except AssertionError as err:
                raise AssertionError("%s / %s packed, device candidates %s: %s" % (fam, name, device, err)) from err
        same_bytes({name: on_device[0]}, {name: on_host[0]}, (fam, name))


@pytest.mark.parametrize("fam", vc.PACKED_AS_ONE_BATCH)
def test_packed_form_of_a_whole_family_from_one_file(fam, packed, tmp_path):
    """many_regions: the reads of all 300 regions in one file, one pack() over every region's start and end, one encode: regions
    of one row (a read that starts on it is not fetched), regions with no read, every matrix on a row that is a multiple of 16,
    every region's reads, sites and votes in its own slice."""
    from pepper_amd.variant.bam import BAM_handler
    oracle = pu.load_restatement()
    every, per_case = vc.packed_batch(family(fam))
    cases = [case for _name, case, _mine in per_case]
    assert len({rules_of(case) for case in cases}) == 1
    bam = str(tmp_path / ("%s.bam" % fam))
    bu.write_bam(bam, [("ctg", cases[-1][1] + 2000)], {0: every}, flush_every=5)
    n_done, region_pairs, counts = packed.pack(BAM_handler(bam), "ctg", [c[0] for c in cases], [c[1] for c in cases], False, 1)
    assert n_done == len(cases)
    windows = [(q.candidate_region_start, q.candidate_region_end) for q in map(vc.params, cases)]
    on_host, on_device, live = _packed_both_ways(packed, [(c[0], c[1]) for c in cases], [c[2] for c in cases], region_pairs, counts,
                                                 rules_of(cases[0]), windows, fam)
    seen = empty = 0
    for k, (name, case, _mine) in enumerate(per_case):
        clipped = bu.restated_get_reads(every, case[0], case[1], False, 1)
        exp = pu.run_variant(oracle, pu.FlatPileup(case[0], case[1], case[2], clipped), vc.params(case))
        assert live[k] == len(clipped), (fam, name)
        for device, outs in ((False, on_host), (True, on_device)):
            try:
                _check(outs[k], exp)
            except AssertionError as err:
                raise AssertionError("%s / %s packed, device candidates %s: %s" % (fam, name, device, err)) from err
        seen += len(exp["candidates"]) > 0
        empty += len(clipped) == 0
    same_bytes(dict(enumerate(on_device)), dict(enumerate(on_host)), fam)
    assert seen >= 50 and empty >= 50


# ---- the per-position tracks ----------------------------------------------------------------------------------------------------
def _window_rows(case):
    q = vc.params(case)
    return max(0, q.candidate_region_start - case[0]), min(case[1], q.candidate_region_end) - case[0]


@pytest.mark.parametrize("fam", sorted(vc.FAMILIES))
def test_depth_track_over_every_row(fam):
    """Bins [0 .. 7] on the thread's handle: the runs of every region equal Coverage.runs_numpy of coverage_cases.depth_numpy over
    the case's reads -- every row, the rows no candidate window shows among them (reads not walked, mapping quality 0) --, and
    the TILE_DEPTH instance of the tile kernel gives candidates and images byte-identical to the plain one."""
    from pepper_amd.variant import Coverage
    from pepper_amd.variant import PEPPER_VARIANT as pv
    plain = run_family(fam)
    check_family(fam, plain)
    for rules, names in groups_of(fam):
        with pv.thread_depth_bins(BINS) as tracks:
            got = dict(zip(names, run_batch(fam, names, rules)))
            region, start, end, which = tracks.depth_runs()
        same_bytes(got, {n: plain[n] for n in names}, (fam, "depth bins set"))
        runs = list(zip(region.tolist(), start.tolist(), end.tolist(), which.tolist()))
        expected = []
        for r, name in enumerate(names):
            case = family(fam)[name]
            depth = depth_numpy(case[3], case[0], case[1], rules[0], rules[1], 1)
            lo, hi = _window_rows(case)
            s, e, k = Coverage.runs_numpy(depth[lo:hi + 1], case[0] + lo, BINS)
            expected += [(r, x, y, z) for x, y, z in zip(s.tolist(), e.tolist(), k.tolist())]
            # the rows only this track shows are within the bins; so are, in the cases of DEPTH_EXACT, the rows the case is about
            assert all(int(depth[row]) <= 7 for row in vc.DEPTH_ONLY[fam, name] if row < len(depth))
            assert name not in vc.DEPTH_EXACT[fam] or all(int(depth[row]) <= 7 for row in vc.EDGES[fam, name])
        assert len(runs) == len(expected) and runs == expected, fam
    same_bytes(run_family(fam), plain, (fam, "depth bins off again"))


@pytest.mark.parametrize("fam", sorted(vc.FAMILIES))
def test_reference_confidence_table_changes_nothing_else(fam):
    """A table set (the TILE_REFCONF instance): candidates and images byte-identical to the plain run; on two families the blocks
    equal RefConfidence's numpy rule over refconf_cases.evidence_numpy, as tests/test_gpu_refconf.py computes it."""
    from pepper_amd.variant import RefConfidence
    from pepper_amd.variant import PEPPER_VARIANT as pv
    table, bands = RefConfidence.build_table(), list(RefConfidence.DEFAULT_BANDS)
    plain = run_family(fam)
    check_family(fam, plain)
    for rules, names in groups_of(fam):
        with pv.thread_ref_confidence(table, bands) as tracks:
            got = dict(zip(names, run_batch(fam, names, rules)))
            merged = RefConfidence.merge_blocks(*tracks.ref_blocks())
        same_bytes(got, {n: plain[n] for n in names}, (fam, "table set"))
        if fam in REFCONF_FAMILIES:
            expected = []
            for r, name in enumerate(names):
                case = family(fam)[name]
                ev = evidence_numpy(case[3], case[2], case[0], case[1], rules[0], rules[1], 1)
                cols = RefConfidence.blocks_numpy(ev[0], RefConfidence.gq_numpy(*ev, table), case[0], bands)
                expected += [(r,) + rec for rec in zip(*(c.tolist() for c in cols))]
            blocks = list(zip(*(c.tolist() for c in merged)))
            assert len(blocks) == len(expected) and blocks == expected, fam
    same_bytes(run_family(fam), plain, (fam, "table off again"))
