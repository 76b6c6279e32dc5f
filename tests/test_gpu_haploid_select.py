"""The device selection with a ploidy (pa_selector_set_ploidy, k_select_decide in pepper_amd/csrc/select.hip) against the host
library over ALL rows (pa_candidates_reference_flags + pa_candidates_select_format_ploidy with the numpy mask of Ploidy.py's
rule): the same rows kept, the same flags (& 0x3d), letters, low-complexity flags and compacted fields, byte for byte -- the
compacted prediction being the MODEL's triple."""
import ctypes

import numpy as np
import pytest
import torch

from haploid_utils import DELETE_AFTER, HET, haploid_case, host_select_ploidy, mask_of, par_table
from pepper_amd import _lib
from pepper_amd.variant import DeviceSelect
from pepper_amd.variant.DeviceSelect import DeviceSelector
from select_utils import Case, contig_text, rules

pytestmark = pytest.mark.gpu

FIELDS = ("row", "flags", "letter", "in_repeat", "position", "depth", "support", "prediction", "name_offsets")
R = 256                                     # DeviceSelector.limits()["rows_per_workgroup"], asserted below
# SNPs by probability only; indels by probability or by a frequency of 0.2 (so that a deletion is kept either way and only
# its swap tells by which)
RULE = dict(p=(0.1, 0.25, 0.25), p_lc=(0.1, 0.25, 0.25), above=(0.0, 0.2, 0.2))


@pytest.fixture(scope="module")
def selector():
    s = DeviceSelector(0)
    yield s
    s.close()


def _run(selector, case, rule):
    return selector.run(rule, case.position, case.depth, case.support, case.prediction, case.blob, case.regions)


def _same(taken, want):
    for field in FIELDS:
        got = getattr(taken, field)
        assert got.dtype == want[field].dtype and got.shape == want[field].shape, field
        assert got.tobytes() == want[field].tobytes(), field
    assert taken.names == want["names"]


def _bytes(taken):
    return b"".join(getattr(taken, f).tobytes() for f in FIELDS) + taken.names


def _changed(case, rule, mask):
    """(rows whose admission or genotype differs between the diploid and the primed decision, rows whose swap differs)."""
    dip, hap = host_select_ploidy(case, rule, None), host_select_ploidy(case, rule, mask)
    state = np.full((2, case.n), -1, np.int64)
    state[0, dip["row"]], state[1, hap["row"]] = dip["flags"] >> 4, hap["flags"] >> 4
    swap = np.zeros((2, case.n), bool)
    swap[0, dip["row"]], swap[1, hap["row"]] = (dip["flags"] & 4) != 0, (hap["flags"] & 4) != 0
    both = (state[0] >= 0) & (state[1] >= 0)
    return int((state[0] != state[1]).sum()), int((both & (swap[0] != swap[1])).sum())


@pytest.mark.parametrize("n", [1, 64, R, R + 1, 3 * R + 17])
@pytest.mark.parametrize("intervals", [0, 1, 2, 37])
def test_device_decides_as_the_host_with_the_mask(selector, n, intervals):
    assert DeviceSelector.limits()["rows_per_workgroup"] == R
    rule = rules(**RULE)
    table = par_table(intervals)
    case = haploid_case(n, 1000 * intervals + n, table)
    if intervals and n >= 64:                               # the rows at the edges of the first and the last interval are there
        edges = {int(table[0][0]) - 1, int(table[0][0]), int(table[1][0]) - 1, int(table[1][0]),
                 int(table[0][-1]) - 1, int(table[0][-1]), int(table[1][-1]) - 1, int(table[1][-1])}
        assert edges <= set(case.position.tolist()) and 0 in case.position.tolist()
    mask = mask_of(table, case.position)
    want = host_select_ploidy(case, rule, mask)
    assert want is not None
    selector.set_ploidy(True, *table)
    try:
        status, m, name_bytes = _run(selector, case, rule)
        assert status == 0 and (m, name_bytes) == (len(want["row"]), len(want["names"]))
        taken = selector.take()
        _same(taken, want)
        assert np.array_equal((taken.flags & 8) != 0, mask[taken.row])
        assert not ((taken.flags[(taken.flags & 8) != 0] >> 4) == 1).any()          # no haploid row is called het
        # the segment's text is the host's over all rows: the formatter primes the compacted MODEL triples again
        assert DeviceSelect.segment(rule, b"c", taken).lines == want["lines"]
        # not vacuous: a quarter of the rows change genotype or admission under priming, and a deletion's swap flips
        changed, swaps = _changed(case, rule, mask)
        print("n %d, %d intervals: %d haploid rows, %d kept, %d change, %d swaps flip" % (n, intervals, mask.sum(), m, changed, swaps))
        assert 4 * changed >= n
        if n >= 64:
            assert swaps >= 1
    finally:
        selector.set_ploidy(False)


def test_threshold_equality_after_priming(selector):
    """(0.125, 0.5, 0.375) primes to non_alt = 0.75: admitted at a threshold of exactly 0.75, not at the next double above; as a
    diploid row (inside the PAR) its non_alt is 0.5 and it is not admitted at either."""
    text = contig_text()
    case = Case([20, 21, 500], [40] * 3, [1] * 3, [HET, DELETE_AFTER, HET], [b"1A", b"3ACG", b"1A"], [(0, 0, text)])
    table = (np.array([400], np.int64), np.array([600], np.int64))
    mask = mask_of(table, case.position)
    assert mask.tolist() == [True, True, False]
    selector.set_ploidy(True, *table)
    try:
        for thr, want_rows in ((0.75, [0]), (float(np.nextafter(0.75, 1.0)), [])):
            rule = rules(p=(thr, 0.25, 2.0), p_lc=(thr, 0.25, 2.0), above=(0.0, 0.0, 0.0))
            want = host_select_ploidy(case, rule, mask)
            assert want["row"].tolist() == want_rows
            status, m, _ = _run(selector, case, rule)
            assert status == 0 and m == len(want_rows)
            _same(selector.take(), want)
        # the deletion: 0.1875 / 0.75 = 0.25 exactly, admitted (and swapped) at 0.25 and not at the next double above
        for thr, want_rows in ((0.25, [1]), (float(np.nextafter(0.25, 1.0)), [])):
            rule = rules(p=(2.0, 2.0, thr), p_lc=(2.0, 2.0, thr), above=(0.0, 0.0, 0.0))
            want = host_select_ploidy(case, rule, mask)
            assert want["row"].tolist() == want_rows and (want["flags"] & 4).tolist() == [4] * len(want_rows)
            assert _run(selector, case, rule)[0] == 0
            _same(selector.take(), want)
    finally:
        selector.set_ploidy(False)


def test_a_nan_row_is_still_handed_back(selector):
    rule = rules(**RULE)
    table = par_table(2)
    case = haploid_case(300, 7, table)
    selector.set_ploidy(True, *table)
    try:
        for column in (0, 1, 2):
            bad = Case(case.position, case.depth, case.support, case.prediction.copy(), case.names, case.regions)
            bad.prediction[5 if column else 0, column] = np.nan          # (row 0 is haploid, row 5 .. whatever it is)
            assert host_select_ploidy(bad, rule, mask_of(table, bad.position)) is None
            status, m, name_bytes = _run(selector, bad, rule)
            assert status == 2 and (m, name_bytes) == (0, 0)             # PA_SELECT_NAN
            with pytest.raises(_lib.PepperAmdError, match="handed back"):
                selector.take()
        assert _run(selector, case, rule)[0] == 0                        # as good as new afterwards
        _same(selector.take(), host_select_ploidy(case, rule, mask_of(table, case.position)))
    finally:
        selector.set_ploidy(False)


def test_switching_it_off_gives_the_never_set_bytes(selector):
    rule = rules(**RULE)
    table = par_table(37)
    case = haploid_case(3 * R + 17, 99, table)
    fresh = DeviceSelector(0)
    try:
        assert _run(fresh, case, rule)[0] == 0
        never = fresh.take()
    finally:
        fresh.close()
    _same(never, host_select_ploidy(case, rule, None))
    assert not (never.flags & 8).any()
    selector.set_ploidy(True, *table)
    assert _run(selector, case, rule)[0] == 0
    on = selector.take()
    assert (on.flags & 8).any() and _bytes(on) != _bytes(never)
    selector.set_ploidy(False)
    assert _run(selector, case, rule)[0] == 0
    assert _bytes(selector.take()) == _bytes(never)
    # the raw entry point's (0, 0, NULL, NULL) does the same, and a table on a diploid contig is refused
    lib = _lib.load()
    starts, ends = table
    _lib.check(lib.pa_selector_set_ploidy(selector.handle, 1, len(starts), ctypes.c_void_p(starts.ctypes.data), ctypes.c_void_p(ends.ctypes.data)))
    assert _run(selector, case, rule)[0] == 0 and _bytes(selector.take()) == _bytes(on)
    assert lib.pa_selector_set_ploidy(selector.handle, 0, len(starts), ctypes.c_void_p(starts.ctypes.data), ctypes.c_void_p(ends.ctypes.data)) != 0
    assert lib.pa_selector_set_ploidy(selector.handle, 1, 2, ctypes.c_void_p(ends.ctypes.data), ctypes.c_void_p(starts.ctypes.data)) != 0
    _lib.check(lib.pa_selector_set_ploidy(selector.handle, 0, 0, None, None))
    selector._ploidy_key = None
    assert _run(selector, case, rule)[0] == 0 and _bytes(selector.take()) == _bytes(never)


def test_device_tensors_and_two_runs(selector):
    rule = rules(**RULE)
    table = par_table(37)
    case = haploid_case(1500, 17, table)
    want = host_select_ploidy(case, rule, mask_of(table, case.position))
    dev = torch.device("cuda", 0)
    tensors = [torch.from_numpy(a).to(dev) for a in (case.position, case.depth, case.support, case.prediction)]
    names = torch.from_numpy(np.frombuffer(case.blob, np.uint8).copy()).to(dev)
    regions = [(first, start, torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(dev)) for first, start, text in case.regions]
    torch.cuda.synchronize()
    other = DeviceSelector(0)
    try:
        other.set_ploidy(True, *table)
        results = []
        for _ in range(2):
            assert other.run(rule, *tensors, names, regions)[0] == 0
            results.append(other.take())
        assert _run(other, case, rule)[0] == 0                           # the host-pointer form on the same selector
        results.append(other.take())
        for taken in results:
            _same(taken, want)
        assert len({_bytes(t) for t in results}) == 1
    finally:
        other.close()
