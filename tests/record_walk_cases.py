"""Hand-built BAM records and spans for the device's record walk (csrc/inflate.hip: record_chase_kernel, record_base_kernel,
record_finish_kernel behind pa_encoder_walk_records): a builder whose every length field can lie, a catalogue of named
cases, and a literal restatement of what the walk must report.

The restatement is derived from the SAM specification (4.2 the record, 4.2.2 the CG tag, 4.2.4 the auxiliary fields) and
from the contract of include/pepper_amd_io.h (pa_record_header) and include/pepper_amd_encoder.h (pa_encoder_walk_records,
pa_encoder_set_split_slices) -- not from the kernels.  Where the specification and the contract differ the contract says
"htslib's rules": an array's subtype is sized with the table of the scalar letters (A and d included, which 4.2.4 does not
list for B), and fewer than four bytes behind the last field are not a field.  Not product code."""
import struct

import numpy as np

import bam_utils as bu
from pepper_amd.variant.bam import BAM_handler, PACKED_READ, RECORD_HEADER

TID, CONTIG = 0, "ctg"
INT32_MAX = 0x7fffffff
# the regions every pack comparison uses: honest records lie in the first two, the nine-N records reach all three
REGION_STARTS, REGION_STOPS = [0, 4000, 1 << 20], [4000, 1 << 20, (1 << 31) - 2]
REF_OPS = (0, 2, 3, 7, 8)                       # M D N = X consume the reference (SAM specification 1.4.6)
AUX_BYTES = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}
N28 = (1 << 28) - 1                             # the longest operation a CIGAR word holds
NINE_N = [(0, 10)] + [(3, N28)] * 9             # 10 + 9 * (2^28 - 1) = 2 415 919 105 reference bases: more than an int32
_POS = -123456                                  # (a record built without a position gets one from its place in the span)


# ---- the restatement -------------------------------------------------------------------------------------------------------
def find_cg(aux):
    """The CG:B,I (or B,i) tag among the auxiliary fields `aux` of one record -> ("found", offset of its operations in aux,
    count), ("none",) or ("malformed", reason).  One field after the other (4.2.4: two tag bytes, a type letter, the value);
    a field that does not fit the bytes that are left, or whose letter is unknown, is malformed."""
    aux = bytes(aux)
    p, n = 0, len(aux)
    while n - p >= 4:
        tag, letter = aux[p:p + 2], chr(aux[p + 2])
        p += 3
        if letter in AUX_BYTES:
            if n - p < AUX_BYTES[letter]:
                return ("malformed", "a fixed-size value cut by the record end")
            p += AUX_BYTES[letter]
        elif letter in "ZH":
            nul = aux.find(b"\0", p)
            if nul < 0:
                return ("malformed", "a string without its NUL")
            p = nul + 1
        elif letter == "B":
            if n - p < 5:
                return ("malformed", "an array cut inside its subtype and count")
            sub, count = chr(aux[p]), struct.unpack_from("<I", aux, p + 1)[0]
            if sub not in AUX_BYTES:
                return ("malformed", "an array of an unknown subtype")
            if count * AUX_BYTES[sub] > n - p - 5:
                return ("malformed", "an array longer than the record")
            if tag == b"CG" and sub in "Ii":
                return ("found", p + 5, count)
            p += 5 + count * AUX_BYTES[sub]
        else:
            return ("malformed", "an unknown type letter")
    return ("none",)


def _ref_len(data, at, n_ops):
    words = np.frombuffer(data, "<u4", n_ops, at).astype(np.int64)
    total = int((words >> 4)[np.isin(words & 15, REF_OPS)].sum())
    return min(total, INT32_MAX)                 # pa_record_header: summed in 64 bits, saturated


def restated_header(data, at, bs, split, reasons=None):
    """The header of the record whose size word lies at `at` (block_size = bs >= 32, the record wholly inside the span)."""
    R = at + 4
    ref_id, pos, l_name, mapq, _bin, n_cig, flag, l_seq_u = struct.unpack_from("<iiBBHHHI", data, R)
    l_seq = l_seq_u - (1 << 32) if l_seq_u >= 1 << 31 else l_seq_u
    o_cig = 32 + l_name
    o_seq = o_cig + 4 * n_cig
    o_aux = o_seq + (l_seq_u + 1) // 2 + l_seq_u
    row = dict(data_off=R + o_cig, ref_id=ref_id, pos=pos, l_seq=l_seq, n_cigar=n_cig, flags=flag | mapq << 16, ref_len=0, state=0,
               block_size=bs)
    if l_seq < 0 or o_aux > bs:
        row["state"] = 2
        if reasons is not None:
            reasons.append("core")
        return row
    first = struct.unpack_from("<I", data, R + o_cig)[0] if n_cig >= 1 else None
    if first is not None and first & 15 == 4 and first >> 4 == l_seq:                # 4.2.2: <l_seq>S in front
        if not split:
            row["state"] = 1
        else:
            verdict = find_cg(data[R + o_aux:R + bs])
            if verdict[0] == "malformed":
                row["state"] = 2
                if reasons is not None:
                    reasons.append(verdict[1])
                return row
            if verdict[0] == "found" and n_cig <= verdict[2] < 1 << 29:
                ops = R + o_aux + verdict[1]
                row.update(state=3, data_off=ops, n_cigar=verdict[2], block_size=ops - (R + o_seq), ref_len=_ref_len(data, ops, verdict[2]))
                return row
    row["ref_len"] = _ref_len(data, R + o_cig, n_cig)
    return row


def restated_walk(data, data_bytes, entries, cap, split, reasons=None):
    """-> (headers: array of RECORD_HEADER, flags [2]) as pa_encoder_walk_records must report them for the span data[:data_bytes]
    (bytes behind data_bytes are resident and never looked at), one lane per entry, at most `cap` records per lane.
    reasons: a list that collects why each state-2 header is one ("core" or find_cg's reason)."""
    data = bytes(data)
    rows, flags = [], [0, 0]
    for i, at in enumerate(entries):
        stop = entries[i + 1] if i + 1 < len(entries) else data_bytes
        n = 0
        while at < stop:
            if data_bytes - at < 4:
                flags[1] = 1
                break
            bs = struct.unpack_from("<I", data, at)[0]
            if bs < 32:
                flags[0] |= 2
                break
            if at + 4 + bs > data_bytes:
                flags[1] = 1
                break
            if n == cap:
                flags[0] |= 1
                break
            rows.append(restated_header(data, at, bs, split, reasons))
            n += 1
            at += 4 + bs
        if i + 1 < len(entries) and at > stop:
            flags[0] |= 8
    out = np.zeros(0 if flags[0] else len(rows), RECORD_HEADER)
    for k in range(len(out)):
        out[k] = tuple(rows[k][name] for name in RECORD_HEADER.names)
    return out, flags


def split_headers(data, data_bytes, first):
    """The headers of a well-formed span walked from its first record with pa_encoder_set_split_slices on."""
    return restated_walk(np.asarray(data).tobytes(), int(data_bytes), [int(first)], 1 << 30, 1)[0]


# ---- the host's own walks over the same span (what the restatement and the device's tables are tied to) ----------------------
READS_CAP, PAIRS_CAP, MIN_MAPQ = 16384, 32768, 1


def contig_handle(directory):
    """A tiny BAM written only for a handle that names the contig."""
    path = str(directory / "tiny.bam")
    bu.write_bam(path, [(CONTIG, (1 << 31) - 1)], {0: [dict(name="t", pos=5, cigar=[(0, 4)], seq="ACGT", qual=[30] * 4)]})
    bam = BAM_handler(path)
    assert bam.contig_index(CONTIG) == TID
    return bam


def host_tables(bam, span, data_bytes, first, headers=None, long_cigars=True):
    """pack_inflated over the span's bytes, or pack_headers over `headers`, a final span and the regions above -> everything
    either returns."""
    reads, pairs = np.zeros(READS_CAP, PACKED_READ), np.zeros(PAIRS_CAP, np.int32)
    args = (CONTIG, REGION_STARTS, REGION_STOPS, False, MIN_MAPQ, reads, pairs)
    if headers is None:
        n_done, region_pairs, counts = bam.pack_inflated(np.frombuffer(span, np.uint8), data_bytes, first, True, *args, long_cigars=long_cigars)
    else:
        table = headers if len(headers) else np.zeros(1, headers.dtype)
        n_done, region_pairs, counts = bam.pack_headers(table, len(headers), True, *args, long_cigars=long_cigars)
    seq_off, n_split = bam.split_offsets(counts[0])
    return dict(n_done=n_done, region_pairs=region_pairs.tolist(), counts=counts, reads=reads[:counts[0]].tobytes(),
                pair_read=pairs[:counts[1]].tolist(), seq_off=seq_off.tolist(), n_split=n_split)


# ---- the builder -----------------------------------------------------------------------------------------------------------
def words(ops):
    return b"".join(struct.pack("<I", (n << 4) | code) for code, n in ops)


def raw_record(pos=_POS, ops=(), n_bases=0, aux=b"", trailing=b"", name=b"r\0", ref_id=TID, mapq=60, flag=0,
               block_size=None, l_read_name=None, n_cigar_op=None, l_seq=None):
    """One record's bytes: `name`, the operations, (n_bases + 1) / 2 + n_bases bytes of bases and qualities, `aux` and
    `trailing` are what is there; block_size, l_read_name, n_cigar_op and l_seq are what the core says (None: the truth)."""
    seq = bytes((37 * k + 0x12) & 0xff for k in range((n_bases + 1) // 2)) + bytes(2 + k % 40 for k in range(n_bases))
    tail = bytes(name) + words(ops) + seq + bytes(aux) + bytes(trailing)
    core = struct.pack("<iiBBHHHIiii", ref_id, pos, len(name) if l_read_name is None else l_read_name, mapq, 4680,
                       len(ops) if n_cigar_op is None else n_cigar_op, flag, (n_bases if l_seq is None else l_seq) & 0xffffffff, -1, -1, 0)
    return struct.pack("<I", len(core) + len(tail) if block_size is None else block_size) + core + tail


def honest(cigar, pos=_POS, long_cigar=False, aux=b"", drop_cg=False, **fields):
    """bam_utils.encode_record of a read whose bases and qualities fit `cigar`."""
    n = sum(length for code, length in cigar if code in (0, 1, 4, 7, 8))
    rec = dict(pos=pos, cigar=list(cigar), seq="".join("ACGT"[(k * 7 + k // 5) % 4] for k in range(n)), qual=[5 + k % 30 for k in range(n)],
               long_cigar=long_cigar, aux=aux, drop_cg=drop_cg, name="h", flag=0, mapq=60)
    rec.update(fields)
    out = bytearray(bu.encode_record(TID, dict(rec, pos=max(0, pos))))
    struct.pack_into("<i", out, 8, pos)
    return bytes(out)


def field(tag, letter, value=b""):
    return tag + letter + value


def array(tag, sub, count, payload=b""):
    return tag + b"B" + sub + struct.pack("<I", count) + payload


def cg_tag(ops, sub=b"I", count=None):
    return array(b"CG", sub, len(ops) if count is None else count, words(ops))


REAL = [(0, 6), (1, 1), (0, 2), (2, 3), (0, 4)]            # 13 bases, 15 reference bases


def placeholder(aux, n_bases=13, core=None, **fields):
    """A record whose core CIGAR is the placeholder of 4.2.2 (<n_bases>S<15>N unless `core` says otherwise) in front of `aux`."""
    return raw_record(ops=[(4, n_bases), (3, 15)] if core is None else core, n_bases=n_bases, aux=aux, **fields)


def join(records, first_pos=100, step=7):
    """The span of `records` back to back -> (bytes, the offset of each).  A record built without a position gets
    first_pos + step * its index: ascending, as a sorted BAM has them."""
    out, starts = bytearray(), []
    for k, rec in enumerate(records):
        rec = bytearray(rec)
        if struct.unpack_from("<i", rec, 8)[0] == _POS:
            struct.pack_into("<i", rec, 8, first_pos + step * k)
        starts.append(len(out))
        out += rec
    return bytes(out), starts


class Case(object):
    """fn() -> (span bytes, data_bytes, entries, cap): the span is what is resident, data_bytes <= its length."""

    def __init__(self, name, fn):
        self.name, self.fn, self._built = name, fn, None

    def build(self):
        if self._built is None:
            span, data_bytes, entries, cap = self.fn()
            assert 0 <= data_bytes <= len(span) < 2 << 20 and cap >= 1 and len(entries) >= 1
            assert all(0 <= a <= data_bytes for a in entries) and all(a < b for a, b in zip(entries, entries[1:]))
            self._built = (bytes(span), int(data_bytes), [int(a) for a in entries], int(cap))
        return self._built

    def __repr__(self):
        return self.name


CASES = []


def case(name):
    def add(fn):
        CASES.append(Case(name, fn))
        return fn
    return add


def one_lane(records, cap=None):
    span, _ = join(records)
    return span, len(span), [0], len(records) if cap is None else cap


def by_name(name):
    return next(c for c in CASES if c.name == name)


# ---- the record core ---------------------------------------------------------------------------------------------------------
@case("l_read_name 0, 1 and 255")
def _():
    return one_lane([raw_record(ops=[(0, 5)], n_bases=5, name=name) for name in (b"", b"\0", b"n" * 254 + b"\0")] +
                    [placeholder(cg_tag(REAL), name=name) for name in (b"", b"\0", b"n" * 254 + b"\0")])


@case("n_cigar_op 0")
def _():
    return one_lane([raw_record(n_bases=4), raw_record(n_bases=4, aux=cg_tag(REAL)), honest([(0, 9)])])


@case("l_seq 0, odd, and 0x80000000")
def _():
    return one_lane([raw_record(ops=[(0, 3)], n_bases=0), raw_record(ops=[(0, 7)], n_bases=7), raw_record(ops=[(0, 1)], n_bases=1),
                     raw_record(ops=[(0, 7)], n_bases=7, l_seq=0x80000000), raw_record(ops=[(4, 0)], n_bases=7, l_seq=0xffffffff),
                     honest([(0, 5)])])


@case("block_size exactly 32")
def _():
    return one_lane([raw_record(name=b""), honest([(0, 3)]), raw_record(name=b"")])


@case("block_size 31")
def _():
    return one_lane([honest([(0, 3)]), raw_record(name=b"", block_size=31), honest([(0, 3)])])


@case("the aux offset equal to block_size, and one beyond it")
def _():
    # bases and qualities of l_seq = 1 take two bytes: a record that ends behind them, and one that holds only one of them
    return one_lane([raw_record(ops=[(0, 1)], n_bases=1), raw_record(ops=[(0, 1)], n_bases=0, trailing=b"\x11", l_seq=1),
                     placeholder(b"", n_bases=1), raw_record(ops=[(4, 1), (3, 9)], n_bases=0, trailing=b"\x11", l_seq=1),
                     raw_record(ops=[(0, 2)], n_bases=2, n_cigar_op=2), honest([(0, 4)])])


# ---- the placeholder rule ----------------------------------------------------------------------------------------------------
@case("placeholder forms")
def _():
    tag = cg_tag(REAL)
    return one_lane([placeholder(tag, core=[(4, 13)]),                       # S of l_seq alone
                     placeholder(tag),                                       # ... with the N operation
                     placeholder(tag, core=[(4, 12), (3, 15)]),              # S of l_seq - 1: no placeholder
                     placeholder(tag, n_bases=0, core=[(4, 0)]),             # l_seq = 0 with 0S
                     placeholder(tag, n_bases=0, core=[(4, 0), (3, 15)]),
                     placeholder(tag, core=[(0, 13), (3, 15)]),              # a first operation that is not S
                     placeholder(tag, core=[(5, 13), (4, 13)]),
                     placeholder(b"")])                                      # no auxiliary field at all


# ---- auxiliary fields: types and layout ----------------------------------------------------------------------------------------
def _value(letter):
    return bytes(range(1, AUX_BYTES[letter] + 1))


@case("every scalar type letter, H, and B of every subtype")
def _():
    recs = [placeholder(field(b"X" + letter.encode(), letter.encode(), _value(letter)) + cg_tag(REAL)) for letter in AUX_BYTES]
    recs.append(placeholder(field(b"XH", b"H", b"1AE301\0") + cg_tag(REAL)))
    recs.append(placeholder(field(b"XH", b"H", b"\0") + cg_tag(REAL)))
    for letter, size in AUX_BYTES.items():
        for count in (0, 1, 3):
            recs.append(placeholder(array(b"XB", letter.encode(), count, bytes(size * count)) + cg_tag(REAL)))
    recs.append(placeholder(b"".join(field(b"Y" + letter.encode(), letter.encode(), _value(letter)) for letter in AUX_BYTES) + cg_tag(REAL)))
    return one_lane(recs)


@case("a B array that fills the record to its last byte, and one element more")
def _():
    recs = []
    for letter, size in AUX_BYTES.items():
        recs.append(placeholder(array(b"XB", letter.encode(), 5, bytes(5 * size))))
        recs.append(placeholder(array(b"XB", letter.encode(), 6, bytes(5 * size))))
    recs.append(placeholder(cg_tag(REAL)))                                   # the tag itself: to the last byte ...
    recs.append(placeholder(cg_tag(REAL, count=len(REAL) + 1)))              # ... and one operation more
    recs.append(placeholder(cg_tag(REAL) + b"\0\0\0"))
    return one_lane(recs)


@case("B counts and subtypes that cannot be")
def _():
    tag = cg_tag(REAL)
    return one_lane([placeholder(array(b"XB", b"d", 0xffffffff, bytes(16)) + tag),      # 2^35 bytes: no 32-bit product
                     placeholder(array(b"XB", b"I", 0x40000000, bytes(16)) + tag),      # 2^32 bytes
                     placeholder(array(b"CG", b"I", 0xffffffff, bytes(16)) + tag),
                     placeholder(array(b"XB", b"Z", 1, b"\0") + tag),                    # an invalid subtype
                     placeholder(array(b"XB", b"B", 1, b"\0") + tag),
                     placeholder(array(b"XB", b"\0", 0) + tag),
                     placeholder(b"XBBI\1\0\0"),                                       # cut inside the count
                     placeholder(b"XBBI"),
                     placeholder(tag)])


@case("a fixed-size value cut by the record end")
def _():
    recs = [placeholder(field(b"XZ", b"Z", b"ab\0") + field(b"X" + letter.encode(), letter.encode(), _value(letter)[:-1]))
            for letter, size in AUX_BYTES.items() if size > 1]
    recs.append(placeholder(field(b"Xd", b"d", b"\1")))
    recs.append(placeholder(field(b"XA", b"A", b"q") + cg_tag(REAL)))
    return one_lane(recs)


@case("an unknown type letter")
def _():
    tag = cg_tag(REAL)
    return one_lane([placeholder(field(b"XX", letter, b"\1\2\3\4") + tag) for letter in (b"q", b"\0", b"z", b"b", b"D", b"\xff")] +
                    [placeholder(tag + field(b"XX", b"q", b"\1\2\3\4")),              # behind the tag: never reached
                     placeholder(field(b"CG", b"q", b"\1\2\3\4") + tag)])


@case("1, 2 and 3 stray bytes behind the last field")
def _():
    recs = []
    for stray in (b"X", b"XY", b"XYq"):
        recs.append(placeholder(field(b"XA", b"A", b"q") + stray))                   # no tag: the core stands
        recs.append(placeholder(cg_tag(REAL) + stray))
        recs.append(placeholder(field(b"XZ", b"Z", b"abc\0") + stray))
        recs.append(placeholder(stray))
    return one_lane(recs)


# ---- auxiliary fields: the CG tag ------------------------------------------------------------------------------------------------
@case("CG tags that are not the one, and the first that is")
def _():
    other = [(0, 1), (2, 40), (0, 12)]
    return one_lane([placeholder(field(b"CG", b"Z", b"13M\0") + cg_tag(REAL)),           # CG as Z: ignored, the walk goes on
                     placeholder(field(b"CG", b"Z", b"13M\0")),
                     placeholder(array(b"CG", b"c", 3, b"\1\2\3") + cg_tag(REAL)),       # CG:B,c in front of the real one
                     placeholder(array(b"CG", b"S", 2, bytes(4)) + array(b"CG", b"f", 1, bytes(4)) + cg_tag(REAL)),
                     placeholder(cg_tag(REAL, sub=b"i")),                                # CG:B,i: accepted
                     placeholder(cg_tag(REAL) + cg_tag(other)),                          # two tags: the first wins
                     placeholder(cg_tag(other) + cg_tag(REAL)),
                     placeholder(field(b"cg", b"i", bytes(4)) + array(b"cG", b"I", 1, bytes(4)) + array(b"Cg", b"I", 1, bytes(4)) + cg_tag(REAL)),
                     placeholder(cg_tag(REAL[:1])),                                      # a count below n_cigar (2)
                     placeholder(cg_tag(REAL[:2])),                                      # ... and equal to it
                     placeholder(cg_tag([])),
                     placeholder(cg_tag(REAL[:1]), core=[(4, 13)])])


# ---- auxiliary fields: strings -----------------------------------------------------------------------------------------------------
@case("a Z string whose NUL sits at every offset around the 64-byte steps of the search")
def _():
    recs = []
    for n in (0, 1, 59, 60, 61, 62, 63, 64, 65, 124, 125, 126, 127, 128, 129, 191, 192, 193):
        recs.append(placeholder(field(b"XZ", b"Z", b"s" * n + b"\0") + cg_tag(REAL)))
        recs.append(placeholder(field(b"XZ", b"Z", b"s" * n + b"\0")))                   # ... as the record's last byte
        recs.append(placeholder(field(b"XZ", b"Z", b"s" * n)))                           # ... and missing
    return one_lane(recs)


@case("a 300 kB Z string")
def _():
    text = bytes(33 + k % 90 for k in range(300000))
    return one_lane([honest([(0, 5)]), placeholder(field(b"MM", b"Z", text + b"\0") + cg_tag(REAL)), placeholder(field(b"MM", b"Z", text)),
                     honest([(0, 6)])])


def _unterminated_then_zeros():
    # the record behind the unterminated string has block_size 256: its size word starts with a zero byte
    follower = raw_record(ops=[(0, 4)], n_bases=4, aux=field(b"XZ", b"Z", b"p" * 208 + b"\0"))
    assert follower[:4] == b"\0\1\0\0"
    return [honest([(0, 8)]), placeholder(field(b"XZ", b"Z", b"no terminator")), follower]


@case("an unterminated Z in front of the next record's zero bytes")
def _():
    return one_lane(_unterminated_then_zeros() + [placeholder(field(b"XH", b"H", b"AB")), raw_record(name=b"", mapq=0)])


@case("an unterminated Z as the last record of a cut span, zero bytes resident behind the cut")
def _():
    span, _ = join(_unterminated_then_zeros()[:2])
    return span + bytes(200), len(span), [0], 2


# ---- reference lengths -------------------------------------------------------------------------------------------------------------
@case("operations of every code with lengths up to 2^28 - 1")
def _():
    recs = [raw_record(ops=[(code, n)], n_bases=3) for code in range(10) for n in (0, 1, N28)]
    recs.append(raw_record(ops=[(code, N28) for code in range(10)], n_bases=3))          # 5 * (2^28 - 1): still an int32
    recs.append(placeholder(cg_tag([(code, N28) for code in range(10)])))
    recs += [raw_record(ops=[(code, 3)], n_bases=3) for code in range(10, 16)]           # codes the specification does not name
    return one_lane(recs)


def _many_ops(n):
    return [((0, 1, 2, 7, 8, 4, 3, 9, 5, 6)[k % 10], 1 + k % 29) for k in range(n)]


@case("operation counts around the 64 lanes of the sum")
def _():
    recs = []
    for n in (1, 2, 63, 64, 65, 100, 127, 128, 129, 200):
        recs.append(raw_record(ops=_many_ops(n), n_bases=5))
        recs.append(placeholder(cg_tag(_many_ops(n))))
    recs.append(raw_record(ops=[(3, 7)] * 64 + [(0, 5)], n_bases=5))                     # all of the sum in the 65th operation's lane 0
    recs.append(raw_record(ops=[(4, 7)] * 128 + [(0, 5)], n_bases=5))
    return one_lane(recs)


@case("nine N operations of 2^28 - 1 bases")
def _():
    return one_lane([raw_record(pos=100, ops=NINE_N, n_bases=10),                         # the core form ...
                     raw_record(pos=101, ops=[(4, 10), (3, N28)], n_bases=10, aux=cg_tag(NINE_N)),      # ... and the CG form
                     raw_record(pos=102, ops=[(0, 10)] + [(3, N28)] * 8, n_bases=10),     # 2^31 - 8 + 10 = 2^31 + 2
                     raw_record(pos=103, ops=[(0, 10)] + [(3, N28)] * 7 + [(2, N28 - 4)], n_bases=10),   # 2^31 - 2: the largest below the cap
                     raw_record(pos=104, ops=[(0, 10)] + [(3, N28)] * 7 + [(2, N28 - 2)], n_bases=10),   # 2^31
                     raw_record(pos=105, ops=[(3, N28)] * 16 + [(0, 10)], n_bases=10),    # 2^32 - 6: wraps a uint32 as well
                     raw_record(pos=106, ops=[(3, N28)] * 17 + [(0, 10)], n_bases=10),
                     honest([(0, 30)], pos=120), honest([(0, 30)], pos=3990), honest([(0, 30)], pos=5000)])


@case("core CIGARs alone: every code, the lane counts, nine N")
def _():
    # no placeholder among them: with split slices off, too, the device's tables are compared with pack_inflated's
    recs = [raw_record(pos=100, ops=NINE_N, n_bases=10), raw_record(pos=101, ops=[(code, N28) for code in range(10)], n_bases=3)]
    recs += [raw_record(pos=102 + k, ops=_many_ops(n), n_bases=5 + k) for k, n in enumerate((1, 63, 64, 65, 127, 128, 129, 1000))]
    recs += [honest([(0, 30)], pos=120), honest([(4, 3), (0, 30)], pos=3990), honest([(0, 30)], pos=5000)]
    return one_lane(recs)


# ---- the structure of a span -------------------------------------------------------------------------------------------------------
ENTRY_COUNTS = [1, 63, 64, 65, 200, 2, 17, 1, 64, 30] * 15              # records per entry of the 150-entry span; the last gets 0


def _structured():
    counts = ENTRY_COUNTS[:149]
    recs, entries, at = [], [], 0
    for i, n in enumerate(counts):
        entries.append(at)
        for k in range(n):
            j = len(recs)
            if j % 11 == 3:
                rec = placeholder(cg_tag(_many_ops(3 + j % 70)) if j % 22 == 3 else field(b"XZ", b"Z", b"t" * (j % 130) + b"\0"))
            else:
                rec = raw_record(ops=[(0, 2 + j % 5), (2, j % 3), (0, 1)], n_bases=3 + j % 5, name=b"s%d\0" % j)
            recs.append(rec)
            at += len(rec)
    span, _ = join(recs, first_pos=50, step=1)
    assert len(span) == at
    return span, entries + [at]


@case("150 entries, the largest count met exactly")
def _():
    span, entries = _structured()
    return span, len(span), entries, max(ENTRY_COUNTS)


@case("150 entries, one slot too few")
def _():
    span, entries = _structured()
    return span, len(span), entries, max(ENTRY_COUNTS) - 1


@case("65 entries of one record each")
def _():
    span, starts = join([raw_record(ops=[(0, 4)], n_bases=4) for _ in range(65)])
    return span, len(span), starts, 1


def _with_a_record_inside():
    """Five records; the third carries, as the payload of a B,C array that ends the record, bytes that read as a record of their
    own ending where the third ends -> (span, starts, the offset of the inner record)."""
    inner = raw_record(pos=114, ops=[(0, 6)], n_bases=6, name=b"inner\0", aux=field(b"XZ", b"Z", b"x\0"))
    outer = raw_record(ops=[(0, 9)], n_bases=9, aux=array(b"XB", b"C", len(inner), inner))
    span, starts = join([honest([(0, 5)]), honest([(0, 6)]), outer, honest([(0, 7)]), placeholder(cg_tag(REAL))])
    return span, starts, starts[3] - len(inner)


@case("an entry in the middle of a record whose walk overshoots the next entry")
def _():
    span, starts, inner = _with_a_record_inside()
    return span, len(span), [0, inner, starts[4]], 8              # lane 0 ends at starts[3], beyond `inner`; lane 1 is clean


@case("a first entry in the middle of a record whose walk re-synchronises")
def _():
    span, starts, inner = _with_a_record_inside()
    return span, len(span), [inner, starts[4]], 8


@case("an entry in the middle of a record that reads as a record shorter than its core")
def _():
    span, starts, _inner = _with_a_record_inside()
    return span, len(span), [0, starts[1] + 4 + 28, starts[3]], 8          # (the template length of the second record: 0)


def _cut(extra):
    span, starts = join([honest([(0, 5)]), placeholder(cg_tag(REAL)), honest([(0, 6)]), honest([(0, 7)]), honest([(0, 8)])])
    return span, starts[3] + extra, [0, starts[2]], 4


for _extra, _what in ((1, "1 byte into a size word"), (3, "3 bytes into a size word"), (4, "4 bytes into a size word: the size word alone"),
                      (30, "in the middle of a record"), (0, "between two records: smaller than the resident span")):
    case("data_bytes cut " + _what)(lambda extra=_extra: _cut(extra))


@case("a last entry equal to data_bytes, behind a cut")
def _():
    span, starts = join([honest([(0, 5)]), honest([(0, 6)]), honest([(0, 7)])])
    return span, starts[2], [0, starts[1], starts[2]], 1


# ---- the random family ---------------------------------------------------------------------------------------------------------------
def _random_aux(rng, lying):
    out = b""
    for _ in range(int(rng.integers(0, 4))):
        kind = int(rng.integers(0, 12))
        letter = "AcCsSiIfd"[kind] if kind < 9 else None
        if letter:
            out += field(b"X" + letter.encode(), letter.encode(), bytes(rng.integers(0, 256, AUX_BYTES[letter], dtype=np.uint8)))
        elif kind == 9:
            out += field(b"XZ", b"ZH"[int(rng.integers(0, 2)):][:1], bytes(rng.integers(1, 256, int(rng.integers(0, 200)), dtype=np.uint8)) + b"\0")
        else:
            sub = "AcCsSiIfd"[int(rng.integers(0, 9))]
            n = int(rng.integers(0, 20))
            out += array(b"CG" if kind == 11 and sub not in "Ii" else b"XB", sub.encode(), n, bytes(rng.integers(0, 256, n * AUX_BYTES[sub], dtype=np.uint8)))
    if not lying:
        return out
    lie = int(rng.integers(0, 8))
    if lie == 0:
        out += field(b"XZ", b"Z", bytes(rng.integers(1, 256, int(rng.integers(0, 150)), dtype=np.uint8)))        # no NUL
    elif lie == 1:
        out += array(b"XB", b"cSId"[int(rng.integers(0, 4)):][:1], int(rng.integers(9, 1 << 32)), bytes(8))
    elif lie == 2:
        out += field(b"XX", bytes([int(rng.choice([0, 33, 66 + 32, 113, 122, 255]))]), bytes(4))
    elif lie == 3:
        out += field(b"Xd", b"d", bytes(int(rng.integers(1, 8))))
    elif lie == 4:
        out += array(b"XB", b"Z", 2, bytes(2))
    return out                                                   # (5 to 7: nothing wrong after all)


def _random_records(seed, n, lying):
    rng = np.random.default_rng(seed)
    recs = []
    for _ in range(n):
        n_bases = int(rng.integers(0, 40))
        real = [(int(rng.integers(0, 10)), int(rng.integers(0, 300))) for _ in range(int(rng.choice([1, 2, 5, 63, 64, 65, 130], p=[.2, .3, .3, .05, .05, .05, .05])))]
        form = int(rng.integers(0, 10))
        name = bytes(rng.integers(33, 127, int(rng.integers(0, 30)), dtype=np.uint8)) + b"\0"
        common = dict(name=name, mapq=int(rng.choice([0, 20, 60])), flag=int(rng.choice([0, 16, 0x100, 0x400, 0x800, 0x4], p=[.5, .3, .05, .05, .05, .05])))
        if form < 4:                                             # a plain record
            lies = {}
            if lying and rng.random() < 0.15:
                which = int(rng.integers(0, 4))
                lies = [dict(l_seq=int(rng.integers(1 << 31, 1 << 32))), dict(l_seq=n_bases + int(rng.integers(1, 1 << 20))),
                        dict(n_cigar_op=len(real) + int(rng.integers(1, 60000))), dict(l_read_name=255)][which]
            recs.append(raw_record(ops=real, n_bases=n_bases, aux=_random_aux(rng, False), **common, **lies))
        else:                                                    # a placeholder
            core = [(4, n_bases), (3, int(rng.integers(0, 5000)))][:int(rng.integers(1, 3))]
            aux = _random_aux(rng, lying and rng.random() < 0.3)
            tag = int(rng.integers(0, 8))
            if tag < 5:
                aux += cg_tag(real, sub=b"Ii"[tag % 2:][:1])
            elif tag == 5:
                aux += cg_tag(real[:len(core) - 1])                # a count below n_cigar
            elif tag == 6 and lying:
                aux += cg_tag(real, count=len(real) + int(rng.integers(1, 1 << 30)))
            aux += (b"", b"", b"X", b"XY", b"XYZ")[int(rng.integers(0, 5))]
            if form == 9:
                core[0] = (4, n_bases + 1)                         # S of another length: no placeholder
            recs.append(raw_record(ops=core, n_bases=n_bases, aux=aux, **common))
    return recs


def _random_span(seed, n, lying):
    span, starts = join(_random_records(seed, n, lying), first_pos=10, step=1)
    entries = starts[::37]
    return span, len(span), entries, 37


@case("random family: honest and lying fields")
def _():
    return _random_span(20261, 2000, True)


@case("random family: honest fields only")
def _():
    return _random_span(20262, 600, False)
