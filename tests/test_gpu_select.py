"""The device selection (pepper_amd/csrc/select.hip through pepper_amd/variant/DeviceSelect.py) against the host library
(pa_candidates_reference_flags + pa_candidates_select_format): the same rows kept, byte for byte the same compacted arrays."""
import numpy as np
import pytest
import torch

from pepper_amd import _lib
from pepper_amd.variant import DeviceSelect, FastCandidates
from pepper_amd.variant.DeviceSelect import DeviceSelector
from select_utils import Case, branches, contig_text, host_select, random_case, rules

pytestmark = pytest.mark.gpu

FIELDS = ("row", "flags", "letter", "in_repeat", "position", "depth", "support", "prediction", "name_offsets")
STATUS = {"zero_depth": 1, "nan": 2, "name": 4, "context": 8, "name_count": 16}


@pytest.fixture(scope="module")
def selector():
    s = DeviceSelector(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def limits():
    return DeviceSelector.limits()


def _run(selector, case, rule, names=None):
    return selector.run(rule, case.position, case.depth, case.support, case.prediction, case.blob if names is None else names, case.regions)


def _same(taken, want):
    for field in FIELDS:
        got = getattr(taken, field)
        assert got.dtype == want[field].dtype and got.shape == want[field].shape, field
        assert got.tobytes() == want[field].tobytes(), field
    assert taken.names == want["names"]


def _check(selector, case, rule):
    """Device against host on one case -> the host's kept rows."""
    want = host_select(case, rule)
    assert want is not None
    status, m, name_bytes = _run(selector, case, rule)
    assert status == 0
    assert (m, name_bytes) == (len(want["row"]), len(want["names"]))
    _same(selector.take(), want)
    return want


def test_limits(limits):
    assert limits["rows_per_workgroup"] == 256 and limits["max_name"] == 64
    assert limits["scan_level"] == limits["scan_block"] * (limits["scan_block"] - 1)


def test_random_rows_take_every_branch(selector):
    """700 rows over three regions (three workgroups, the last one partly filled).  First the host's own result: it keeps between a
    fifth and four fifths of the rows and takes every branch of the rules."""
    rule = rules(p=(0.75, 0.65, 0.85), p_lc=(0.9, 0.5, 0.95))
    case = random_case(700, seed=11)
    want = host_select(case, rule)
    seen = branches(case, rule, want)
    assert 0.2 * case.n <= seen["kept"] <= 0.8 * case.n, seen
    for key in ("kind0", "kind1", "kind2", "by_probability", "by_probability_lc", "by_frequency", "swap", "unswapped_delete",
                "refused_letter", "refused_allele", "type_outside", "genotype0", "genotype1", "genotype2"):
        assert seen[key] > 0, (key, seen)
    text = contig_text()
    assert any(65 <= c <= 90 for c in want["letter"]) and (np.frombuffer(text, np.uint8)[want["position"]] >= 97).any()      # (a lower-case base kept)
    status, m, _ = _run(selector, case, rule)
    assert status == 0 and m == seen["kept"]
    _same(selector.take(), want)


def test_sizes(selector, limits):
    """Rows: 0, 1, one wave, one workgroup and one scan block of rows, each -1 / +0 / +1."""
    rule = rules()
    wg, block = limits["rows_per_workgroup"], limits["scan_block"]
    for n in (0, 1, 63, 64, 65, wg - 1, wg, wg + 1, block - 1, block, block + 1):
        _check(selector, random_case(n, seed=100 + n), rule)


def test_name_bytes_cross_the_same_edges(selector, limits):
    """The scan over the names' bytes: exactly one wave, one workgroup and one scan block of bytes, each -1 / +0 / +1."""
    rule = rules()
    for k, total in enumerate(sorted({e + d for e in (64, limits["rows_per_workgroup"], limits["scan_block"]) for d in (-1, 0, 1)})):
        case = random_case(total // 6, seed=200 + k, name_bytes=total)
        assert len(case.blob) == total
        _check(selector, case, rule)


@pytest.mark.parametrize("extra", [0, 1])
def test_scan_top_level(selector, limits, extra):
    """The largest input whose scan of the name bytes needs no further level (scan_level bytes), and the smallest that does."""
    total = limits["scan_level"] + extra
    case = random_case(200000 - extra, seed=300 + extra, name_bytes=total)
    assert len(case.blob) == total
    _check(selector, case, rules())


def test_rows_past_one_scan_block_of_workgroups(selector, limits):
    """One row more than scan_block workgroups hold: the scan of the workgroups' totals takes two blocks (and the names, more than
    scan_level bytes of them, the further level)."""
    case = random_case(limits["rows_per_workgroup"] * limits["scan_block"] + 1, seed=310)
    assert len(case.blob) > limits["scan_level"]
    _check(selector, case, rules())


# ---- hand-built edges --------------------------------------------------------------------------------------------------------
def _rows(text, rows, ref0=0):
    """rows: (position, depth, support, (p0, p1, p2), name) over one region whose reference is `text` from ref0."""
    return Case([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows],
                [(0, ref0, text)])


def _kept_rows(selector, case, rule):
    return _check(selector, case, rule)["row"].tolist()


PLAIN = b"ACGTCAGTGCATGACTAGCTAGTCAGCTAGCATCGATGCATCGTAGCTAGCATGCATCGAT"     # no run of 2: nothing is low complexity


def test_threshold_exact_and_one_ulp(selector):
    """non_alt whose double equals the threshold, and the float32 values next to it."""
    thr = np.float32(0.3)
    below, above = np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1))
    rule = rules(p=(float(thr), float(thr), float(thr)), p_lc=(2.0, 2.0, 2.0), above=(0.0, 0.0, 0.0))
    rows = [(20 + k, 10, 1, (0.1, float(v), 0.0), name) for k, (v, name) in enumerate(
        [(below, b"1A"), (thr, b"1A"), (above, b"1A"), (below, b"2AC"), (thr, b"2AC"), (thr, b"3AC"), (below, b"3AC")])]
    assert _kept_rows(selector, _rows(PLAIN, rows), rule) == [1, 2, 4, 5]
    # the threshold as a double that no float32 equals: the float32 on either side of it
    rule = rules(p=(0.3, 0.3, 0.3), p_lc=(2.0, 2.0, 2.0), above=(0.0, 0.0, 0.0))
    rows = [(20, 10, 1, (0.0, float(np.float32(0.3)), 0.0), b"1A"), (21, 10, 1, (0.0, float(np.nextafter(np.float32(0.3), np.float32(0))), 0.0), b"1A")]
    assert float(np.float32(0.3)) > 0.3
    assert _kept_rows(selector, _rows(PLAIN, rows), rule) == [0]


def test_frequency_admission_edges(selector):
    """support / depth against report_above_freq: equal (1/4 against 0.25), beside it (1/3 against 0.3333333333333333 and its
    neighbours), and report_above_freq of 0 and below, which admit nothing."""
    third = 1.0 / 3.0
    low = (0.9, 0.0, 0.0)                  # (nothing is admitted by probability: the thresholds are 2)
    for above, want in ((0.25, [0, 2]), (third, [2]), (float(np.nextafter(third, 0.0)), [2]), (float(np.nextafter(third, 1.0)), []),
                        (0.0, []), (-0.5, [])):
        rule = rules(p=(2.0, 2.0, 2.0), p_lc=(2.0, 2.0, 2.0), above=(above, above, above))
        rows = [(20, 4, 1, low, b"1A"), (21, 5, 1, low, b"2AC"), (22, 3, 1, low, b"3ACG"), (23, 1000, 1, low, b"1C")]
        assert _kept_rows(selector, _rows(PLAIN, rows), rule) == want, above
    # a deletion admitted by frequency is not swapped; admitted by probability it is
    rule = rules(p=(0.5, 0.5, 0.5), p_lc=(0.5, 0.5, 0.5), above=(0.2, 0.2, 0.2))
    case = _rows(PLAIN, [(20, 4, 1, low, b"3ACG"), (21, 4, 1, (0.1, 0.8, 0.1), b"3ACG"), (22, 4, 1, (0.1, 0.8, 0.1), b"3A")])
    want = _check(selector, case, rule)
    assert (want["flags"] & 4).tolist() == [0, 4, 4] and (want["flags"] & 1).tolist() == [0, 0, 1]


def test_ties_among_probabilities(selector):
    rule = rules(p=(0.0, 0.0, 0.0), p_lc=(0.0, 0.0, 0.0))
    preds = [(0.5, 0.5, 0.5), (0.2, 0.5, 0.5), (0.5, 0.2, 0.5), (0.5, 0.5, 0.2), (0.1, 0.2, 0.3), (0.3, 0.2, 0.1), (0.0, 0.0, 0.0),
             (-0.0, 0.0, -0.0), (float("inf"), float("inf"), 1.0)]
    want = _check(selector, _rows(PLAIN, [(20 + k, 9, 3, p, b"1G") for k, p in enumerate(preds)]), rule)
    assert (want["flags"] >> 4).tolist() == [0, 1, 0, 0, 2, 0, 0, 0, 0]


def test_context_cut_at_both_ends(selector):
    """Positions 0, 4, 9 and 10 of a contig (the context is cut at 0) and the last ten positions of a reference that ends."""
    rule = rules(p=(0.5, 0.5, 0.5), p_lc=(0.9, 0.9, 0.9), above=(0.0, 0.0, 0.0))
    text = b"AAAAACGTCAGTGCATGACTAGCTAGTCAGCTAGCATCGATGCATCGTAGCTCCCCC"
    rows = [(p, 9, 3, (0.1, 0.7, 0.0), b"1T") for p in (0, 4, 9, 10, 11)] + \
           [(p, 9, 3, (0.1, 0.7, 0.0), b"1T") for p in range(len(text) - 10, len(text) + 1)]
    want = _check(selector, _rows(text, rows), rule)
    # the run [0, 5) touches [p - 5, p + 4) up to p = 9 and is cut to four letters from p = 11 on; the run at the end touches
    # from p = len - 8 on; the last row lies behind the reference
    assert want["repeat"].tolist() == [1, 1, 1, 0, 0] + [0, 0] + [1] * 8 + [0] and want["letters"].tolist()[-1] == 0
    assert want["row"].tolist() == [3, 4, 5, 6]
    # the same reference as a region that does not start at 0: positions with ten bases in front of them
    case = _rows(text, [(100 + p, 9, 3, (0.1, 0.95, 0.0), b"1T") for p in (10, 11, 20, len(text) - 1)], ref0=100)
    _check(selector, case, rule)


def test_runs_of_exactly_five(selector):
    """A run of exactly 5 that ends at p - 5 (outside the touched stretch), one that starts at p + 3 (inside), one at p + 4
    (outside); the same with runs of 4, which never count."""
    rule = rules(p=(0.5, 0.5, 0.5), p_lc=(2.0, 2.0, 2.0), above=(0.0, 0.0, 0.0))
    p = 30
    seen = []
    for run, start in ((5, p - 10), (5, p - 9), (5, p + 3), (5, p + 4), (4, p - 2), (6, p + 4), (6, p - 11), (7, p - 11), (5, p + 6)):
        text = bytearray(PLAIN)
        text[start:start + run] = b"T" * run
        if text[start - 1] == ord("T"):
            text[start - 1] = ord("C")
        if text[start + run] == ord("T"):
            text[start + run] = ord("C")
        want = _check(selector, _rows(bytes(text), [(p, 9, 3, (0.1, 0.7, 0.0), b"1G")]), rule)
        seen.append(int(want["repeat"][0]))
    # ends at p - 5, ends at p - 4, starts at p + 3, starts at p + 4, a run of 4, 6 from p + 4; 6 from p - 11 (five of them inside the
    # context, ending at p - 5), 7 from p - 11 (six inside), 5 from p + 6 (four inside)
    assert seen == [0, 1, 1, 0, 0, 0, 0, 1, 0]


def test_longest_name_all_kept_none_kept(selector, limits):
    rule = rules(p=(0.0, 0.0, 0.0), p_lc=(0.0, 0.0, 0.0))
    longest = b"2" + b"ACGT" * 15 + b"ACG"
    assert len(longest) == limits["max_name"]
    rows = [(20 + k, 9, 3, (0.1, 0.7, 0.0), name) for k, name in enumerate((longest, b"1A", b"3" + longest[1:], b"1"))]
    want = _check(selector, _rows(PLAIN, rows * 100), rule)
    assert len(want["row"]) == 400                                           # all kept
    rule = rules(p=(2.0, 2.0, 2.0), p_lc=(2.0, 2.0, 2.0), above=(0.0, 0.0, 0.0))
    want = _check(selector, _rows(PLAIN, rows * 100), rule)
    assert len(want["row"]) == 0                                             # none kept


# ---- handed back -------------------------------------------------------------------------------------------------------------
def _handed_back(selector, case, rule, status, names=None):
    got, m, name_bytes = _run(selector, case, rule, names)
    assert got == STATUS[status] and (m, name_bytes) == (0, 0)
    with pytest.raises(_lib.PepperAmdError, match="handed back"):
        selector.take()


class _Fasta(object):
    """get_reference_sequence over one contig, as FastCandidates' reference window asks for it."""

    def __init__(self, text):
        self.text = text.decode()

    def get_chromosome_sequence_length(self, contig):
        return len(self.text)

    def get_reference_sequence(self, contig, start, stop):
        return self.text[max(0, start):stop]


def _native(case, rule):
    from types import SimpleNamespace
    return FastCandidates.native_batch_arrays(SimpleNamespace(), rule, _Fasta(case.regions[0][2]), b"c", case.n, case.position, case.depth,
                                              case.support.reshape(-1, 1), case.prediction, case.blob)


def test_handed_back_cases(selector, limits):
    rule = rules()
    good = (20, 9, 3, (0.1, 0.7, 0.0), b"1A")
    nan = float("nan")
    # a valid-allele row with depth 0 (whatever its type character), a NaN probability: the host library returns -2
    for row, status in (((21, 0, 3, (0.1, 0.7, 0.0), b"2AC"), "zero_depth"), ((21, 0, 0, (0.1, 0.7, 0.0), b"7AC"), "zero_depth"),
                        ((21, 9, 3, (nan, 0.7, 0.0), b"1A"), "nan"), ((21, 9, 3, (0.1, 0.7, nan), b"3AC"), "nan")):
        case = _rows(PLAIN, [good, row, good])
        assert host_select(case, rule) is None and _native(case, rule) is None
        _handed_back(selector, case, rule, status)
    # ... and neither is one where the host never gets that far: a refused letter, a refused allele, a type outside '1'..'3' (NaN)
    case = _rows(PLAIN + b"N", [good, (len(PLAIN), 0, 3, (nan, nan, nan), b"1A"), (22, 0, 3, (nan, nan, nan), b"1N"), (23, 9, 3, (nan, 0.1, 0.1), b"5A")])
    assert _check(selector, case, rule)["row"].tolist() == [0]
    # names: empty, a list byte (in a row of any kind): native_batch_arrays returns None
    for name in (b"", b"1A,C", b"[1A", b"1 A", b"1'A", b'1"A', b"1A]", b"1\nA"):
        case = _rows(PLAIN, [good, (21, 9, 3, (0.1, 0.7, 0.0), name), good])
        assert _native(case, rule) is None
        _handed_back(selector, case, rule, "name")
    # ... longer than the limit
    case = _rows(PLAIN, [good, (21, 9, 3, (0.1, 0.7, 0.0), b"2" + b"A" * limits["max_name"]), good])
    _handed_back(selector, case, rule, "name")
    # a context that starts in front of the reference given, which does not start at the contig's start
    case = _rows(PLAIN, [(100 + 9, 9, 3, (0.1, 0.7, 0.0), b"1A")], ref0=100)
    _handed_back(selector, case, rule, "context")
    _check(selector, _rows(PLAIN, [(100 + 10, 9, 3, (0.1, 0.7, 0.0), b"1A"), (99, 9, 3, (0.1, 0.7, 0.0), b"1A")], ref0=100), rule)
    # a count of NULs other than n: one too few, one too many
    case = _rows(PLAIN, [good, good, good])
    assert _native(Case(case.position, case.depth, case.support, case.prediction, [b"1A", b"1A"], case.regions), rule) is None
    _handed_back(selector, case, rule, "name_count", names=b"1A\x001A\x001A")
    _handed_back(selector, case, rule, "name_count", names=b"1A\x001A\x001A\x00\x00")
    # the selector is as good as new afterwards
    _check(selector, case, rule)


# ---- device pointers, repeated runs -------------------------------------------------------------------------------------------
def test_device_pointers_and_two_runs(selector):
    rule = rules()
    case = random_case(1500, seed=17)
    want = _check(selector, case, rule)
    dev = torch.device("cuda", 0)
    tensors = [torch.from_numpy(a).to(dev) for a in (case.position, case.depth, case.support, case.prediction)]
    names = torch.from_numpy(np.frombuffer(case.blob, np.uint8).copy()).to(dev)
    regions = [(first, start, torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(dev)) for first, start, text in case.regions]
    torch.cuda.synchronize()
    other = DeviceSelector(0)
    try:
        results = []
        for _ in range(2):
            status, m, name_bytes = other.run(rule, *tensors, names, regions)
            assert status == 0
            results.append(other.take())
        for taken in results:
            _same(taken, want)
    finally:
        other.close()


def test_segment_is_the_hosts(selector):
    """DeviceSelect.segment over a taken result: the lines, len(REF), snp and sel native_batch_arrays gives for the full lists."""
    rule = rules()
    text = contig_text()
    full = random_case(900, seed=23)
    case = Case(full.position[:300], full.depth[:300], full.support[:300], full.prediction[:300], full.names[:300], [(0, 0, text)])
    want = host_select(case, rule)
    assert _run(selector, case, rule)[0] == 0
    seg = DeviceSelect.segment(rule, b"c", selector.take())
    assert seg.lines == want["lines"] and seg.contig == "c"
    assert seg.pos.tolist() == want["position"].tolist() and seg.ref_len.tolist() == want["ref_len"].tolist()
    assert seg.snp.tolist() == (want["full_flags"] & 1).astype(bool).tolist() and seg.sel.tolist() == (want["full_flags"] & 2).astype(bool).tolist()
    native = _native(case, rule)
    assert native.lines == seg.lines and [native.record(k) for k in range(len(seg))] == [seg.record(k) for k in range(len(seg))]
