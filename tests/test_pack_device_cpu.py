"""PackedEncoder.pack_device's ladder without a GPU: a scripted stand-in library and BAM handler answer what a scenario tells
them to (the walk's return code and flags, the pack summary, a BamError, the contig's index, what read_span finds at each number
of regions) and record every call in order.  Each scenario holds the call to its trace, its return value, every counter it
leaves behind and the lap keys it wrote.  tests/test_device_pack_cpu.py imports _encoder, _FakeLib and _FakeBam from here."""
import ctypes

import numpy as np
import pytest

from pepper_amd import _lib
from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
from pepper_amd.variant.bam import BamError


def test_error_codes_mirror_the_header():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pepper_amd.h")).read()
    for name, value in re.findall(r"#define (PA_(?:OK|ERR_\w+)) (\d+)", header):
        assert getattr(_lib, name) == int(value), name


class Script(object):
    """What the stand-ins answer; a scenario overrides what it is about."""
    has_index = True
    host_span = True                # pa_encoder_host_span gives a block
    span = (0, 4096)                # region_span's begin and end
    read_span = {}                  # regions in the call -> (complete, out_bytes); any other number: (True, 1000)
    walk_rc = 0                     # of pa_encoder_walk_records / pa_encoder_submit_walk
    walk_flags = (0, 0)
    n_headers = 7
    contig_index = 2
    status = 0                      # the pack summary's
    device_split = 0                # ... and its n_split
    headers_error = None            # the BamError code pack_headers / pack_inflated raises
    inflated_error = None
    n_reads = 3                     # what the host packers count
    n_split = 0                     # of split_offsets
    download_flags = None           # the flags pa_encoder_walk_headers reports, where they differ from the submitted walk's

    def __init__(self, **over):
        for key, value in over.items():
            assert hasattr(Script, key), key
            setattr(self, key, value)
        self.trace = []


class _FakeLib(object):
    """The entry points pack_device needs without the device pack (tests/test_device_pack_cpu.py counts on that)."""

    def __init__(self, walk_rc, script=None):
        self.script = script if script is not None else Script(walk_rc=walk_rc)
        self.trace = self.script.trace
        self.calls = []

    def pa_encoder_host_span(self, enc, cap):
        self.trace.append(("host_span",))
        if not self.script.host_span:
            return None
        self.buf = np.zeros(cap, np.uint8)
        return self.buf.ctypes.data

    def pa_encoder_inflate_bgzf(self, *a):
        self.calls.append("inflate")
        self.trace.append(("inflate", a[-1] is not None))
        return 0

    def pa_encoder_last_timing(self, enc, ptr, n):
        (ctypes.c_double * n).from_address(ptr)[10] = 2.0
        return 0

    def pa_encoder_set_split_slices(self, enc, on):
        self.trace.append(("set_split_slices", on))
        return 0

    def _walked(self, n_headers, flags_ptr):
        n_headers._obj.value = self.script.n_headers
        (ctypes.c_int32 * 2).from_address(flags_ptr)[:] = self.script.walk_flags

    def pa_encoder_walk_records(self, *a):
        self.calls.append("walk")
        self.trace.append(("walk_records",))
        if self.script.walk_rc == 0:
            self._walked(a[7], a[8])
        return self.script.walk_rc


class _PackLib(_FakeLib):
    """... and the three of the device pack."""

    def pa_encoder_submit_walk(self, *a):
        self.trace.append(("submit_walk",))
        return self.script.walk_rc

    def pa_encoder_pack_records(self, enc, headers, n_headers, final, tid, n, starts, stops, supp, min_mapq, max_reads, max_pairs,
                                pairs, summary):
        self.trace.append(("pack_records", tid, n, tuple((ctypes.c_int64 * n).from_address(starts))))
        (ctypes.c_int32 * (n + 1)).from_address(pairs)[:] = list(range(n + 1))
        s = summary._obj
        s.status, s.n_done, s.n_reads, s.n_pairs, s.n_split = self.script.status, n, 5, 6, self.script.device_split
        s.walk_flags[0], s.walk_flags[1] = self.script.walk_flags
        return 0

    def pa_encoder_walk_headers(self, enc, headers, cap, n_headers, flags):
        self.trace.append(("walk_headers",))
        self._walked(n_headers, flags)
        if self.script.download_flags is not None:
            (ctypes.c_int32 * 2).from_address(flags)[:] = self.script.download_flags
        return 0


def _bam_error(code):
    err = BamError("scripted %d" % code)
    err.code = code
    return err


class _FakeBam(object):
    def __init__(self, script=None):
        self.script = script if script is not None else Script()
        self.trace = self.script.trace

    def has_index(self):
        return self.script.has_index

    def region_span(self, contig, start, stop, lookahead):
        self.n = stop // 1000                       # (the scenarios' regions end at 1000, 2000, ...)
        self.trace.append(("region_span", self.n))
        return self.script.span[0], 0, self.script.span[1], True

    def read_span(self, begin, end, span, tables, flag):
        self.trace.append(("read_span",))
        complete, out_bytes = self.script.read_span.get(self.n, (True, 1000))
        return 1, 100, out_bytes, complete, True

    def span_entries(self, contig, first, out_off, n_blocks, entries):
        self.trace.append(("span_entries",))
        return 1

    def contig_index(self, contig):
        self.trace.append(("contig_index",))
        return self.script.contig_index

    def _packed(self, error, starts):
        if error is not None:
            raise _bam_error(error)
        n = len(starts)
        return n, np.arange(n + 1, dtype=np.int32), (self.script.n_reads, 2 * self.script.n_reads, 999)

    def pack_headers(self, headers, n_headers, final, contig, starts, stops, supp, min_mapq, reads, pair_read, long_cigars=False):
        self.trace.append(("pack_headers", n_headers, tuple(int(s) for s in starts), bool(long_cigars)))
        return self._packed(self.script.headers_error, starts)

    def pack_inflated(self, data, data_bytes, first, final, contig, starts, stops, supp, min_mapq, reads, pair_read, long_cigars=False):
        self.trace.append(("pack_inflated", tuple(int(s) for s in starts), bool(long_cigars)))
        return self._packed(self.script.inflated_error, starts)

    def split_offsets(self, n_reads):
        self.trace.append(("split_offsets", n_reads))
        self.seq_off = np.arange(n_reads, dtype=np.int64)
        return self.seq_off, self.script.n_split

    def pack_regions(self, contig, starts, stops, supp, min_mapq, arena, reads, pair_read):
        self.trace.append(("pack_regions",))
        return self._packed(None, starts)


def _encoder(walk_rc, script=None):
    enc = object.__new__(PackedEncoder)
    enc.lib = _FakeLib(walk_rc) if script is None else _PackLib(walk_rc, script)
    enc.enc = ctypes.c_void_p()
    enc.device = 0
    enc.arena = np.zeros(1 << 16, np.uint8)
    enc.reads, enc.pair_read = np.zeros(8, np.int64), np.zeros(16, np.int32)
    enc.span = enc.tables = enc.headers = enc.entries = None
    enc.inflate_ms, enc.inflated_bytes = 0.0, 0
    enc.seq_off, enc.long_cigar_reads = None, 0
    enc.close = lambda: None
    return enc


def test_stale_index_sends_the_batch_to_the_host_packer(monkeypatch):
    monkeypatch.setenv("PEPPER_AMD_DEVICE_WALK", "1")
    enc = _encoder(_lib.PA_ERR_INVALID)
    got = enc.pack_device(_FakeBam(), "chr20", np.array([0]), np.array([1000]), False, 1)
    assert got is None and enc.lib.calls == ["inflate", "walk"]


def test_any_other_walk_error_is_raised(monkeypatch):
    monkeypatch.setenv("PEPPER_AMD_DEVICE_WALK", "1")
    enc = _encoder(_lib.PA_ERR_HIP)
    with pytest.raises(_lib.PepperAmdError) as info:
        enc.pack_device(_FakeBam(), "chr20", np.array([0]), np.array([1000]), False, 1)
    assert info.value.code == _lib.PA_ERR_HIP


# ---- the ladder -------------------------------------------------------------------------------------------------------------

STARTS = np.array([0, 1000, 2000, 3000])
STOPS = STARTS + 1000
S4, S2, S1 = (0, 1000, 2000, 3000), (0, 1000), (0,)
COUNTERS = dict(host_walk_spans=0, pack_handbacks=0, long_cigar_reads=0, device_packed=False, seq_off=None, inflated_bytes=0)
SPAN, INFLATE, WALK_DEVICE, WALK = "bam_span_read", "bam_inflate_device", "bam_walk_device", "bam_walk"


def fit(*ns):
    """The calls of the span fit that tries these numbers of regions in turn."""
    return [call for n in ns for call in (("region_span", n), ("read_span",))]


def host_packed(n=4, n_reads=3, out_bytes=1000):
    return n, list(range(n + 1)), (n_reads, 2 * n_reads, out_bytes)


def call(monkeypatch, script, walk="1", enc=None, **kw):
    """One pack_device call of four regions -> (encoder, what it returned or the exception it raised, laps)."""
    monkeypatch.setenv("PEPPER_AMD_DEVICE_WALK", walk)
    if enc is None:
        enc = _encoder(script.walk_rc, script)
    else:
        enc.lib.script = script
        enc.lib.trace = script.trace
    laps = {}
    try:
        got = enc.pack_device(_FakeBam(script), "chr20", STARTS, STOPS, False, 1, laps=laps, **kw)
    except (BamError, _lib.PepperAmdError) as err:
        got = err
    return enc, got, laps


def hold(enc, script, got, laps, trace, returns, lap_keys, **counters):
    assert script.trace == trace
    if isinstance(returns, tuple) and len(returns) == 2 and returns[0] == "raises":
        assert isinstance(got, Exception) and got.code == returns[1], got
    elif returns is None:
        assert got is None
    else:
        assert not isinstance(got, Exception), got
        assert (got[0], list(got[1]), tuple(got[2])) == returns
    want = dict(COUNTERS, **counters)
    have = dict(host_walk_spans=enc.host_walk_spans, pack_handbacks=enc.pack_handbacks, long_cigar_reads=enc.long_cigar_reads,
                device_packed=enc.device_packed, seq_off=None if enc.seq_off is None else list(enc.seq_off),
                inflated_bytes=enc.inflated_bytes)
    assert have == want
    assert enc.inflate_ms == 2.0 * enc.lib.calls.count("inflate")       # (the stand-in's 2 ms per inflate)
    assert set(laps) == set(lap_keys) and all(v >= 0.0 for v in laps.values())


DEVICE_WALK = [("host_span",)] + fit(4) + [("inflate", False), ("span_entries",)]
SUBMITTED = DEVICE_WALK + [("contig_index",), ("submit_walk",), ("pack_records", 2, 4, S4)]
REINFLATED = [("inflate", True), ("pack_inflated", S4, False)]

# name, script, pack_device's keywords and PEPPER_AMD_DEVICE_WALK, trace, return value, lap keys, counters that are not COUNTERS'
LADDER = [
    ("no index", dict(has_index=False), {}, [], None, [], {}),
    ("no page-locked block for the span", dict(host_span=False), {}, [("host_span",)], None, [], {}),
    ("empty span", dict(span=(4096, 4096)), {}, [("host_span",)] + fit(4)[:1], (4, [0] * 5, (0, 0, 0)), [], {}),
    ("the span fits at two regions", dict(read_span={4: (True, 1 << 16)}), {},
     [("host_span",)] + fit(4, 2) + [("inflate", False), ("span_entries",), ("walk_records",), ("pack_headers", 7, S2, False)],
     host_packed(2), [SPAN, INFLATE, WALK_DEVICE, WALK], dict(inflated_bytes=1000)),
    ("the span fits at one region: incomplete at four, 255 bytes of slack at two",
     dict(read_span={4: (False, 1000), 2: (True, (1 << 16) - 255), 1: (True, (1 << 16) - 256)}), dict(walk="0"),
     [("host_span",)] + fit(4, 2, 1) + [("inflate", True), ("pack_inflated", S1, False)],
     host_packed(1, out_bytes=(1 << 16) - 256), [SPAN, INFLATE, WALK], dict(inflated_bytes=(1 << 16) - 256)),
    ("the span never fits", dict(read_span={4: (False, 1000), 2: (False, 1000), 1: (False, 1000)}), {},
     [("host_span",)] + fit(4, 2, 1), None, [], {}),
    ("PEPPER_AMD_DEVICE_WALK=0", {}, dict(walk="0"), [("host_span",)] + fit(4) + [("inflate", True), ("pack_inflated", S4, False)],
     host_packed(), [SPAN, INFLATE, WALK], dict(inflated_bytes=1000)),
    ("PEPPER_AMD_DEVICE_WALK=0 leaves device_pack and long_cigars=False without a library call", {},
     dict(walk="0", device_pack=True), [("host_span",)] + fit(4) + [("inflate", True), ("pack_inflated", S4, False)],
     host_packed(), [SPAN, INFLATE, WALK], dict(inflated_bytes=1000)),
    ("device walk, flags clear", {}, {}, DEVICE_WALK + [("walk_records",), ("pack_headers", 7, S4, False)],
     host_packed(), [SPAN, INFLATE, WALK_DEVICE, WALK], dict(inflated_bytes=1000)),
    ("device walk, flags set", dict(walk_flags=(1, 0)), {}, DEVICE_WALK + [("walk_records",)] + REINFLATED,
     host_packed(), [SPAN, INFLATE, WALK_DEVICE, WALK], dict(inflated_bytes=2000, host_walk_spans=1)),
    ("the walk reports a stale index", dict(walk_rc=_lib.PA_ERR_INVALID), {}, DEVICE_WALK + [("walk_records",)],
     None, [SPAN, INFLATE], dict(inflated_bytes=1000)),
    ("the walk fails otherwise", dict(walk_rc=_lib.PA_ERR_HIP), {}, DEVICE_WALK + [("walk_records",)],
     ("raises", _lib.PA_ERR_HIP), [SPAN, INFLATE], dict(inflated_bytes=1000)),
    ("pack_headers -6 under long_cigars", dict(headers_error=-6), dict(long_cigars=True),
     DEVICE_WALK + [("set_split_slices", 1), ("walk_records",), ("pack_headers", 7, S4, True), ("inflate", True),
                         ("pack_inflated", S4, True), ("split_offsets", 3)],
     host_packed(), [SPAN, INFLATE, WALK_DEVICE, WALK], dict(inflated_bytes=2000, host_walk_spans=1)),
    ("pack_headers -6 without long_cigars", dict(headers_error=-6), {},
     DEVICE_WALK + [("walk_records",), ("pack_headers", 7, S4, False)], ("raises", -6),
     [SPAN, INFLATE, WALK_DEVICE, WALK], dict(inflated_bytes=1000)),
    ("pack_inflated -6 under long_cigars", dict(inflated_error=-6), dict(walk="0", long_cigars=True),
     [("host_span",)] + fit(4) + [("inflate", True), ("pack_inflated", S4, True)], ("raises", -6),
     [SPAN, INFLATE, WALK], dict(inflated_bytes=1000)),
] + [
    ("pack_headers %d" % code, dict(headers_error=code), {}, DEVICE_WALK + [("walk_records",), ("pack_headers", 7, S4, False)],
     None if code != -5 else ("raises", -5), [SPAN, INFLATE, WALK_DEVICE, WALK], dict(inflated_bytes=1000))
    for code in (-7, -8, -9, -5)
] + [
    ("pack_inflated %d" % code, dict(inflated_error=code), dict(walk="0"),
     [("host_span",)] + fit(4) + [("inflate", True), ("pack_inflated", S4, False)],
     None if code != -5 else ("raises", -5), [SPAN, INFLATE, WALK], dict(inflated_bytes=1000))
    for code in (-7, -8, -9, -5)
] + [
    ("pack_inflated -8 behind pack_headers -6", dict(headers_error=-6, inflated_error=-8), dict(long_cigars=True),
     DEVICE_WALK + [("set_split_slices", 1), ("walk_records",), ("pack_headers", 7, S4, True), ("inflate", True),
                         ("pack_inflated", S4, True)],
     None, [SPAN, INFLATE, WALK_DEVICE, WALK], dict(inflated_bytes=2000, host_walk_spans=1)),
    ("long_cigars, reads, none split", {}, dict(walk="0", long_cigars=True),
     [("host_span",)] + fit(4) + [("inflate", True), ("pack_inflated", S4, True), ("split_offsets", 3)],
     host_packed(), [SPAN, INFLATE, WALK], dict(inflated_bytes=1000)),
    ("long_cigars, two reads split", dict(n_split=2), dict(walk="0", long_cigars=True),
     [("host_span",)] + fit(4) + [("inflate", True), ("pack_inflated", S4, True), ("split_offsets", 3)],
     host_packed(), [SPAN, INFLATE, WALK], dict(inflated_bytes=1000, seq_off=[0, 1, 2], long_cigar_reads=2)),
    ("long_cigars, no reads", dict(n_reads=0, n_split=2), dict(walk="0", long_cigars=True),
     [("host_span",)] + fit(4) + [("inflate", True), ("pack_inflated", S4, True)],
     host_packed(n_reads=0), [SPAN, INFLATE, WALK], dict(inflated_bytes=1000)),
    ("device pack", {}, dict(device_pack=True), SUBMITTED, (4, list(range(5)), (5, 6, 1000)), [SPAN, INFLATE, WALK_DEVICE],
     dict(inflated_bytes=1000, device_packed=True)),
    ("device pack of split reads under long_cigars", dict(device_split=3, n_split=9), dict(device_pack=True, long_cigars=True),
     DEVICE_WALK + [("set_split_slices", 1)] + SUBMITTED[-3:], (4, list(range(5)), (5, 6, 1000)), [SPAN, INFLATE, WALK_DEVICE],
     dict(inflated_bytes=1000, device_packed=True, long_cigar_reads=3)),
    ("device pack of split reads without long_cigars", dict(device_split=3), dict(device_pack=True), SUBMITTED,
     (4, list(range(5)), (5, 6, 1000)), [SPAN, INFLATE, WALK_DEVICE], dict(inflated_bytes=1000, device_packed=True)),
    ("device pack handed back", dict(status=3), dict(device_pack=True), SUBMITTED + [("walk_headers",), ("pack_headers", 7, S4, False)],
     host_packed(), [SPAN, INFLATE, WALK_DEVICE, WALK], dict(inflated_bytes=1000, pack_handbacks=1)),
    ("device pack handed back, then pack_headers -7", dict(status=3, headers_error=-7), dict(device_pack=True),
     SUBMITTED + [("walk_headers",), ("pack_headers", 7, S4, False)], None, [SPAN, INFLATE, WALK_DEVICE, WALK],
     dict(inflated_bytes=1000, pack_handbacks=1)),
    ("device pack, walk flags set", dict(walk_flags=(1, 0)), dict(device_pack=True), SUBMITTED + REINFLATED,
     host_packed(), [SPAN, INFLATE, WALK_DEVICE, WALK], dict(inflated_bytes=2000, host_walk_spans=1)),
    ("device pack, walk flags set and handed back", dict(walk_flags=(1, 0), status=3), dict(device_pack=True), SUBMITTED + REINFLATED,
     host_packed(), [SPAN, INFLATE, WALK_DEVICE, WALK], dict(inflated_bytes=2000, host_walk_spans=1)),
    ("device pack, the header download sets the flags", dict(status=3, download_flags=(1, 0)), dict(device_pack=True),
     SUBMITTED + [("walk_headers",)] + REINFLATED, host_packed(), [SPAN, INFLATE, WALK_DEVICE, WALK],
     dict(inflated_bytes=2000, host_walk_spans=1, pack_handbacks=1)),
    ("device pack, stale index", dict(walk_rc=_lib.PA_ERR_INVALID), dict(device_pack=True), SUBMITTED[:-1],
     None, [SPAN, INFLATE], dict(inflated_bytes=1000)),
    ("device pack, another walk error", dict(walk_rc=_lib.PA_ERR_HIP), dict(device_pack=True), SUBMITTED[:-1],
     ("raises", _lib.PA_ERR_HIP), [SPAN, INFLATE], dict(inflated_bytes=1000)),
    ("device pack, the header does not name the contig", dict(contig_index=-1), dict(device_pack=True),
     DEVICE_WALK + [("contig_index",), ("walk_records",), ("pack_headers", 7, S4, False)],
     host_packed(), [SPAN, INFLATE, WALK_DEVICE, WALK], dict(inflated_bytes=1000)),
    ("device pack, no contig index", dict(contig_index=None), dict(device_pack=True),
     DEVICE_WALK + [("contig_index",), ("walk_records",), ("pack_headers", 7, S4, False)],
     host_packed(), [SPAN, INFLATE, WALK_DEVICE, WALK], dict(inflated_bytes=1000)),
]


@pytest.mark.parametrize("name,script,how,trace,returns,lap_keys,counters", LADDER, ids=[row[0] for row in LADDER])
def test_ladder(monkeypatch, name, script, how, trace, returns, lap_keys, counters):
    script = Script(**script)
    enc, got, laps = call(monkeypatch, script, **dict(dict(walk="1"), **how))
    hold(enc, script, got, laps, trace, returns, lap_keys, **counters)


def test_the_walk_switch_is_read_per_call(monkeypatch):
    """... and the span and its tables are allocated once."""
    first = Script()
    enc, got, laps = call(monkeypatch, first, walk="0")
    hold(enc, first, got, laps, [("host_span",)] + fit(4) + [("inflate", True), ("pack_inflated", S4, False)], host_packed(),
         [SPAN, INFLATE, WALK], inflated_bytes=1000)
    second = Script()
    enc, got, laps = call(monkeypatch, second, walk="1", enc=enc)
    hold(enc, second, got, laps, DEVICE_WALK[1:] + [("walk_records",), ("pack_headers", 7, S4, False)], host_packed(),
         [SPAN, INFLATE, WALK_DEVICE, WALK], inflated_bytes=2000)
    third = Script()
    enc, got, laps = call(monkeypatch, third, walk="0", enc=enc)
    hold(enc, third, got, laps, fit(4) + [("inflate", True), ("pack_inflated", S4, False)], host_packed(), [SPAN, INFLATE, WALK],
         inflated_bytes=3000)


def test_split_slices_are_sent_when_the_wanted_state_changes(monkeypatch):
    sent = []
    enc = None
    for long_cigars in (True, True, False, False, True):
        script = Script()
        enc, got, _ = call(monkeypatch, script, enc=enc, long_cigars=long_cigars)
        assert got[0] == 4
        sent.append([c for c in script.trace if c[0] == "set_split_slices"])
    assert sent == [[("set_split_slices", 1)], [], [("set_split_slices", 0)], [], [("set_split_slices", 1)]]
    # the host walk sends nothing: the handler's packers are told per call
    script = Script()
    call(monkeypatch, script, walk="0", enc=enc, long_cigars=False)
    assert not [c for c in script.trace if c[0] == "set_split_slices"]


def test_counters_add_up_over_calls(monkeypatch):
    enc = None
    for script, kw in ((Script(walk_flags=(1, 0)), {}), (Script(status=3), dict(device_pack=True)),
                       (Script(headers_error=-6, n_split=2), dict(long_cigars=True)),
                       (Script(device_split=4), dict(long_cigars=True, device_pack=True)), (Script(walk_flags=(1, 0)), {})):
        enc, got, _ = call(monkeypatch, script, enc=enc, **kw)
        assert got[0] == 4
    assert (enc.host_walk_spans, enc.pack_handbacks, enc.long_cigar_reads) == (3, 1, 6)
    assert enc.inflated_bytes == 8000 and enc.seq_off is None and not enc.device_packed


def left_behind(monkeypatch):
    """An encoder after a device pack and one after a host pack of split reads: what the next call has to clear."""
    script = Script()
    packed, got, _ = call(monkeypatch, script, device_pack=True)
    assert packed.device_packed and got[0] == 4
    script = Script(n_split=1)
    split, got, _ = call(monkeypatch, script, long_cigars=True)
    assert split.seq_off is not None and got[0] == 4
    return packed, split


def test_pack_clears_what_an_earlier_call_left(monkeypatch):
    for enc in left_behind(monkeypatch):
        script = Script()
        got = enc.pack(_FakeBam(script), "chr20", STARTS, STOPS, False, 1)
        assert script.trace == [("pack_regions",)] and got[0] == 4
        assert enc.seq_off is None and not enc.device_packed


@pytest.mark.parametrize("script", [dict(has_index=False), dict(span=(7, 7)), dict(read_span={4: (False, 0), 2: (False, 0), 1: (False, 0)}),
                                    dict(walk_rc=_lib.PA_ERR_INVALID), dict(headers_error=-8)],
                         ids=["no index", "empty span", "no fit", "stale index", "does not fit the tables"])
def test_a_pack_device_that_returns_early_clears_it_too(monkeypatch, script):
    for enc in left_behind(monkeypatch):
        script_ = Script(**script)
        enc, got, _ = call(monkeypatch, script_, enc=enc)
        assert got is None or got[2] == (0, 0, 0)
        assert enc.seq_off is None and not enc.device_packed
