"""The device's BAM record walk (csrc/inflate.hip: record_chase_kernel, record_base_kernel, record_finish_kernel with
wave_find_cg) on the hand-built records and spans of tests/record_walk_cases.py: the one place where untrusted bytes compute
device addresses.  Every case goes to the device through the product's own entry points -- raw-DEFLATE members of at most
60 000 bytes through pa_encoder_inflate_bgzf (host_out = NULL), then pa_encoder_set_split_slices and pa_encoder_walk_records,
or pa_encoder_submit_walk + pa_encoder_pack_records(headers = NULL) + pa_encoder_walk_headers -- and must return, bit for bit,
the flags, the count and the 40-byte headers the restatement derives from the SAM specification and the documented contract.
Exact integer parity: no tolerances.

What tests/test_record_walk_cpu.py pins about the catalogue (over both settings of split, so that this test cannot pass by
never reaching a branch): each of the states 0, 1, 2 and 3 at least 20 times (17 190, 2 178, 623 and 1 081 when this was
written); each of the flags[0] bits 1, 2 and 8 and flags[1] at least once (2, 4, 4 and 8 walks); state 2 from the core
(l_seq < 0, fields beyond block_size) and from each reason of the tag walk -- a fixed-size value cut by the record end, a
string without its NUL, an array cut inside its subtype and count, an array of an unknown subtype, an array longer than the
record, an unknown type letter -- at least once, in hand-written cases as well as in the random family.  flags[0] bit 4 (more
records than headers_cap) is set by the host side of the call and is asserted here, in test_headers_cap.

What became of the 2^31 case: record_finish_kernel summed a record's reference bases in a 32-bit int.  Nine N operations of
2^28 - 1 bases (2 415 919 105 bases) wrapped it negative, pa_pack::read_end then gave pos + 1, and the record was a read of its
first region only where pa_bam_pack_inflated's 64-bit sum makes it a read of all three.  The kernel now sums in 64 bits and
saturates ref_len at INT32_MAX (include/pepper_amd_io.h states the rule, the restatement follows it); pa_bam_pack_headers
needed no change, since no region starts at or beyond 2^31 - 1.  test_submitted_walk_and_device_pack compares the tables.
Measured with the kernel as it was: ref_len -1879048191 for the record, 12 tests of this module failed (the two nine-N cases
and a lying record of the random family whose operations add up to more than 2^31 as well).

Deliberate breaks, each tried once on a scratch copy of inflate.hip against this module (not committed):
    - the `at < end` guard dropped from the Z search: 10 tests failed -- the NUL offsets around the 64-byte steps, the
      300 kB string, the unterminated Z in front of the next record's zero bytes and the one at the cut with zero bytes
      resident behind it, the random family (split = 1 of each, walk_records and the submitted walk)
    - `carry = readlane(incl, 63)` instead of `+=` in record_base_kernel: 10 failed -- the 150-entry span and the 65 entries
      of one record each, test_headers_cap, test_walks_repeat_and_reuse_the_workspace
    - `bs < 33` in record_chase_kernel: 8 failed -- "block_size exactly 32" and the 32-byte record behind the unterminated Z
    - `cnt > n_cigar` instead of `>=`: 8 failed -- "CG tags that are not the one" (a count equal to n_cigar), the operation
      counts around 64 (a tag of two operations), both random families
    - the finish loop striding 63 instead of 64: NOTHING failed, and nothing can: wavefront w still reaches every record
      j = w + 63 k, so each record is finished by two wavefronts that store the same 40 bytes.  The break costs time, not
      correctness.  Striding 65, which does skip records (j = 64 for one), failed 6 tests: the 150-entry span (lanes of 65
      and 200 records), test_headers_cap, test_walks_repeat_and_reuse_the_workspace.
"""
import ctypes
import zlib

import numpy as np
import pytest

import deflate_writer as dw
import record_walk_cases as rw
from pepper_amd import _lib
from pepper_amd.bgzf import block_table
from pepper_amd.variant.bam import BamError, PACKED_READ, RECORD_HEADER

pytestmark = pytest.mark.gpu

MEMBER = 60000
_restated = {}


def restated(case, split):
    if (case.name, split) not in _restated:
        span, data_bytes, entries, cap = case.build()
        _restated[case.name, split] = rw.restated_walk(span, data_bytes, entries, cap, split)
    return _restated[case.name, split]


def members_of(span):
    """The span as BGZF members: stored blocks and zlib's streams in turn."""
    out = []
    for k, at in enumerate(range(0, len(span), MEMBER)):
        chunk = span[at:at + MEMBER]
        if k % 2:
            stream = dw.Deflate().stored(chunk, final=True).getvalue()
        else:
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            stream = c.compress(chunk) + c.flush()
        out.append(dw.bgzf_member(stream, chunk))
    return b"".join(out)


class Rig(object):
    def __init__(self):
        self.lib = _lib.load()
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.pa_encoder_create(0, None, ctypes.byref(self.h)))
        self.resident = None

    def close(self):
        self.lib.pa_encoder_destroy(self.h)

    def load(self, case):
        """The case's span resident on the device (once per case in a row)."""
        span, data_bytes, entries, cap = case.build()
        if self.resident != case.name:
            buf = members_of(span)
            comp = np.frombuffer(buf, np.uint8)
            comp_off, comp_len, out_off, out_len = block_table(buf)
            assert int(out_off[-1]) + int(out_len[-1]) == len(span) and int(out_len.max()) <= MEMBER
            _lib.check(self.lib.pa_encoder_inflate_bgzf(self.h, comp.ctypes.data, comp.size, len(comp_off), comp_off.ctypes.data,
                                                        comp_len.ctypes.data, out_off.ctypes.data, out_len.ctypes.data, len(span), None))
            self.resident = case.name
        return data_bytes, np.asarray(entries, np.int64), cap

    def split(self, on):
        _lib.check(self.lib.pa_encoder_set_split_slices(self.h, int(on)))

    def walk(self, case, split, cap=None, headers_cap=None):
        """pa_encoder_walk_records -> (headers [n], flags)."""
        data_bytes, entries, case_cap = self.load(case)
        self.split(split)
        cap = case_cap if cap is None else cap
        room = len(entries) * cap if headers_cap is None else headers_cap
        headers = np.frombuffer(bytearray(b"\x5a" * (40 * max(1, room))), RECORD_HEADER)
        n, flags = ctypes.c_int64(-1), np.full(2, -1, np.int32)
        _lib.check(self.lib.pa_encoder_walk_records(self.h, data_bytes, entries.ctypes.data, len(entries), cap, headers.ctypes.data,
                                                    room, ctypes.byref(n), flags.ctypes.data))
        assert 0 <= n.value <= room
        assert headers[n.value:].tobytes() == b"\x5a" * (40 * (len(headers) - n.value)), "%s: bytes behind the headers written" % case.name
        return headers[:n.value], flags.tolist()

    def submit_and_pack(self, case, split):
        """pa_encoder_submit_walk + pa_encoder_pack_records(headers = NULL) + pa_encoder_walk_headers -> (summary, region_pairs,
        headers [n], flags)."""
        data_bytes, entries, cap = self.load(case)
        self.split(split)
        _lib.check(self.lib.pa_encoder_submit_walk(self.h, data_bytes, entries.ctypes.data, len(entries), cap))
        starts, stops = np.asarray(rw.REGION_STARTS, np.int64), np.asarray(rw.REGION_STOPS, np.int64)
        summary, region_pairs = _lib.DevicePack(), np.full(len(starts) + 1, -5, np.int32)
        _lib.check(self.lib.pa_encoder_pack_records(self.h, None, 0, 1, rw.TID, len(starts), starts.ctypes.data, stops.ctypes.data, 0,
                                                    rw.MIN_MAPQ, rw.READS_CAP, rw.PAIRS_CAP, region_pairs.ctypes.data, ctypes.byref(summary)))
        room = len(entries) * cap
        headers = np.zeros(max(1, room), RECORD_HEADER)
        n, flags = ctypes.c_int64(-1), np.full(2, -1, np.int32)
        _lib.check(self.lib.pa_encoder_walk_headers(self.h, headers.ctypes.data, room, ctypes.byref(n), flags.ctypes.data))
        return summary, region_pairs, headers[:n.value], flags.tolist()

    def packed_tables(self, summary):
        reads, pair_read = np.zeros(max(1, summary.n_reads), PACKED_READ), np.zeros(max(1, summary.n_pairs), np.int32)
        seq_off = np.zeros(max(1, summary.n_reads), np.int64)
        _lib.check(self.lib.pa_encoder_packed_tables(self.h, reads.ctypes.data, pair_read.ctypes.data, seq_off.ctypes.data))
        return reads[:summary.n_reads], pair_read[:summary.n_pairs], seq_off[:summary.n_reads]


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


@pytest.fixture(scope="module")
def handle(tmp_path_factory):
    bam = rw.contig_handle(tmp_path_factory.mktemp("record_walk"))
    yield bam
    bam.close()


def same_headers(name, got, want):
    """Equal bytes, or a failure that names the case and shows the first differing record's fields."""
    assert len(got) == len(want), "%s: %d headers from the device, %d restated" % (name, len(got), len(want))
    if got.tobytes() == want.tobytes():
        return
    k = next(k for k in range(len(want)) if got[k].tobytes() != want[k].tobytes())
    fields = ["%s: device %d, restated %d" % (f, int(got[k][f]), int(want[k][f])) for f in RECORD_HEADER.names if got[k][f] != want[k][f]]
    print("%s, record %d\n  device   %s\n  restated %s" % (name, k, got[k], want[k]))
    pytest.fail("%s: record %d of %d differs (%s)" % (name, k, len(want), "; ".join(fields)))


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("case", rw.CASES, ids=[c.name for c in rw.CASES])
def test_walk_records(rig, case, split):
    want, want_flags = restated(case, split)
    got, flags = rig.walk(case, split)
    assert flags == want_flags, case.name
    same_headers(case.name, got, want)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("case", rw.CASES, ids=[c.name for c in rw.CASES])
def test_submitted_walk_and_device_pack(rig, handle, case, split):
    want, want_flags = restated(case, split)
    summary, region_pairs, got, flags = rig.submit_and_pack(case, split)
    assert [summary.walk_flags[0], summary.walk_flags[1]] == want_flags and flags == want_flags, case.name
    same_headers(case.name, got, want)                       # (the headers fetched afterwards)
    if want_flags[0] != 0:
        assert summary.status == 6 and summary.n_done == 0 and not region_pairs.any(), case.name
        return
    assert summary.n_headers == len(want), case.name
    states = set(want["state"].tolist())
    if 2 in states:
        assert summary.status == 2, case.name               # (every record of the catalogue lies in front of the last stop)
        return
    span, data_bytes, entries, _cap = case.build()
    if 1 in states:
        # split slices off and a placeholder among the records: status 3 where the filters keep one (pa_bam_pack_headers: -8),
        # else the tables pa_bam_pack_headers builds from the restated headers (pack_inflated would look the tag up)
        try:
            tables = rw.host_tables(handle, span, data_bytes, entries[0], want, long_cigars=False)
        except BamError as err:
            assert err.code == -8 and summary.status == 3, (case.name, err.code, summary.status)
            return
    else:
        tables = rw.host_tables(handle, span, data_bytes, entries[0], long_cigars=bool(split))
    assert summary.status == 0, (case.name, summary.status)
    assert (summary.n_done, summary.n_reads, summary.n_pairs, summary.slice_bytes) == (tables["n_done"],) + tuple(tables["counts"]), case.name
    assert region_pairs.tolist() == tables["region_pairs"] and summary.n_split == tables["n_split"], case.name
    reads, pair_read, seq_off = rig.packed_tables(summary)
    assert reads.tobytes() == tables["reads"], case.name
    assert pair_read.tolist() == tables["pair_read"] and seq_off.tolist() == tables["seq_off"], case.name


def test_the_comparisons_above_are_not_vacuous():
    """The cases whose device-built tables test_submitted_walk_and_device_pack compares with pack_inflated's, counted from
    the restatement alone: clean flags and neither state 1 nor state 2."""
    compared = {0: [], 1: []}
    for case in rw.CASES:
        for split in (0, 1):
            want, flags = restated(case, split)
            if flags[0] == 0 and not set(want["state"].tolist()) & {1, 2}:
                compared[split].append(case.name)
    # (with split slices off every placeholder is state 1: few cases are without one, the core form of the nine-N record among them)
    assert len(compared[1]) >= 20 and set(compared[0]) <= set(compared[1]), compared
    for name in ("core CIGARs alone: every code, the lane counts, nine N", "65 entries of one record each", "block_size exactly 32"):
        assert name in compared[0], name
    for name in ("nine N operations of 2^28 - 1 bases", "150 entries, the largest count met exactly", "random family: honest fields only"):
        assert name in compared[1], name


def test_headers_cap(rig):
    """headers_cap equal to the number of records, and one less: flags[0] bit 4, no header."""
    case = rw.by_name("150 entries, the largest count met exactly")
    for split in (0, 1):
        want, want_flags = restated(case, split)
        assert want_flags == [0, 0] and len(want) > 7000
        got, flags = rig.walk(case, split, headers_cap=len(want))
        assert flags == [0, 0]
        same_headers(case.name, got, want)
        got, flags = rig.walk(case, split, headers_cap=len(want) - 1)
        assert flags == [4, 0] and len(got) == 0


def test_walks_repeat_and_reuse_the_workspace(rig):
    """Two walks of one span on one handle leave the same bytes; a small span walked with another cap behind a large one
    shows none of the large one's headers; and the large one comes back unchanged."""
    big, small = rw.by_name("150 entries, the largest count met exactly"), rw.by_name("placeholder forms")
    for split in (1, 0):
        first, flags_a = rig.walk(big, split)
        again, flags_b = rig.walk(big, split)
        assert flags_a == flags_b == [0, 0] and first.tobytes() == again.tobytes()
        same_headers(big.name, first, restated(big, split)[0])
        for cap in (8, 11, 300):
            got, flags = rig.walk(small, split, cap=cap)
            want, want_flags = restated(small, split)
            assert flags == want_flags == [0, 0]
            same_headers(small.name, got, want)
        again, _flags = rig.walk(big, split, cap=201)
        assert again.tobytes() == first.tobytes()


def test_host_pack_refuses_what_the_device_marks(rig, handle):
    """The headers the DEVICE delivers for the cases with a state-2 record make pa_bam_pack_headers fail with -6, as the
    restated ones do in tests/test_record_walk_cpu.py."""
    tried = 0
    for name in ("l_seq 0, odd, and 0x80000000", "an unknown type letter", "a fixed-size value cut by the record end"):
        case = rw.by_name(name)
        got, flags = rig.walk(case, 1)
        assert flags[0] == 0 and (got["state"] == 2).any()
        span, data_bytes, entries, _cap = case.build()
        with pytest.raises(BamError) as e:
            rw.host_tables(handle, span, data_bytes, entries[0], got)
        assert e.value.code == -6
        tried += 1
    assert tried == 3
