"""A DEFLATE writer for tests (RFC 1951) and a catalogue of hand-built streams.

An encoder writes a narrow and always valid slice of the format; this module writes a stream at the level of its symbols, so
that a test can place every construct the RFC allows -- and the ones it forbids -- exactly.  Plain Python and numpy, no GPU:
tests/test_deflate_writer_cpu.py pins the writer and every verdict of the catalogue against zlib, tests/
test_gpu_inflate_crafted.py gives the same streams to the device (csrc/inflate.hip).

  BitWriter                     bits LSB first, Huffman codes MSB first (RFC 1951 3.1.1)
  canonical_codes(lengths)      code assignment of 3.2.2
  Deflate                       block emitters (stored / fixed / dynamic) and symbol emitters; keeps the bytes the stream
                                claims to produce (`out`)
  complete_lengths(rng, n)      a random Kraft-complete set of code lengths
  bgzf_member(stream, payload)  the 18-byte BGZF header, the stream, crc32(payload), len(payload)
  VALID, INVALID                the catalogue: named cases, built on demand (`case.build()`)
  random_member(rng)            one random valid stream of 1 to 4 blocks; RANDOM_SEED / RANDOM_MEMBERS are what the tests run
"""
import struct
import zlib

import numpy as np

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k // 2 for k in range(2, 28)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]          # RFC 1951 3.2.7
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
END = 256


class BitWriter(object):
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def nbits(self):
        return 8 * len(self.buf) + self.n

    def bits(self, v, n):
        """n bits of v, least significant first."""
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """A Huffman code: most significant bit first."""
        rev = 0
        for k in range(length):
            rev |= ((code >> k) & 1) << (length - 1 - k)
        self.bits(rev, length)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.buf += data

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc & 0xff]) if self.n else b"")


def canonical_codes(lengths):
    """{symbol: (code, length)} of every symbol with a non-zero length (RFC 1951 3.2.2).  An over-subscribed set still gets
    numbers (cut to the code's length): such a stream is written to be refused."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for sym, l in enumerate(lengths):
        if l:
            out[sym] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return out


def kraft(lengths):
    """Sum of 2^-length over the codes, in units of 2^-15: 32768 is a complete set."""
    return sum(1 << (15 - l) for l in lengths if l)


def lens_of(spec, n):
    """{symbol: length} -> list of n lengths."""
    out = [0] * n
    for s, l in spec.items():
        out[s] = l
    return out


def complete_with(spec, n, pad):
    """lens_of(spec, n) made Kraft-complete with codes for the symbols of `pad`, one per set bit of what is left."""
    out = lens_of(spec, n)
    left = 32768 - kraft(out)
    assert left >= 0
    pad = list(pad)
    for b in range(14, -1, -1):
        if left >> b & 1:
            s = pad.pop(0)
            assert out[s] == 0
            out[s] = 15 - b
    assert kraft(out) == 32768
    return out


def complete_lengths(rng, n_symbols, max_len=15):
    """A random Kraft-complete set of n_symbols code lengths, none above max_len: from one leaf at depth 0, split a random leaf
    of depth below max_len until there are n_symbols leaves; which symbol gets which leaf is shuffled."""
    if n_symbols < 2 or n_symbols > (1 << max_len):
        raise ValueError("no complete code of %d symbols within %d bits" % (n_symbols, max_len))
    leaves = [0]
    while len(leaves) < n_symbols:
        open_ = [k for k, d in enumerate(leaves) if d < max_len]
        k = open_[int(rng.integers(len(open_)))]
        leaves[k] += 1
        leaves.append(leaves[k])
    return [int(l) for l in rng.permutation(np.asarray(leaves))]


def length_symbol(length):
    """(symbol, extra bits' value) of a match length, the canonical form: 258 is symbol 285."""
    assert 3 <= length <= 258
    if length == 258:
        return 285, 0
    s = max(k for k in range(28) if LENGTH_BASE[k] <= length)
    return 257 + s, length - LENGTH_BASE[s]


def distance_symbol(distance):
    assert 1 <= distance <= 32768
    s = max(k for k in range(30) if DIST_BASE[k] <= distance)
    return s, distance - DIST_BASE[s]


def rle_items(lens):
    """The code length sequence of a dynamic header in run-length form: a plain length 0..15, or (16, n) repeat the previous
    length n = 3..6 times, (17, n) n = 3..10 zeros, (18, n) n = 11..138 zeros."""
    items, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                n = min(run, 138)
                items.append((18, n))
                run -= n
            if run >= 3:
                items.append((17, run))
                run = 0
            items += [0] * run
        else:
            items.append(v)
            run -= 1
            while run >= 3:
                n = min(run, 6)
                items.append((16, n))
                run -= n
            items += [v] * run
        i = j
    return items


def expand_items(items):
    """The lengths a well-formed item list stands for."""
    lens = []
    for it in items:
        if isinstance(it, tuple):
            sym, n = it
            lens += [lens[-1] if sym == 16 else 0] * n
        else:
            lens.append(it)
    return lens


class Deflate(object):
    """One raw DEFLATE stream, block by block and symbol by symbol.  `out` is what the stream claims to produce (a match that
    reaches in front of the output copies zeros; symbols without a meaning add nothing)."""

    def __init__(self):
        self.w = BitWriter()
        self.out = bytearray()
        self.lit = self.dist = None
        self.blocks = []                 # "stored" / "fixed" / "dynamic", in order
        self.longest_lit = self.longest_dist = 0      # the longest codes a symbol of the stream was written with

    def getvalue(self):
        return self.w.getvalue()

    # ---- blocks ----
    def stored(self, data=b"", final=False, length=None, nlen=None):
        """Any LEN (`length`: the field, where it is not len(data)), optionally a wrong NLEN."""
        self.w.bits(1 if final else 0, 1)
        self.w.bits(0, 2)
        self.w.align()
        n = len(data) if length is None else length
        self.w.bits(n, 16)
        self.w.bits(n ^ 0xffff if nlen is None else nlen, 16)
        self.w.raw(data)
        self.out += data
        self.lit = self.dist = None
        self.blocks.append("stored")
        return self

    def reserved(self, final=False):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(3, 2)
        return self

    def fixed(self, final=False):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(1, 2)
        self.lit, self.dist = canonical_codes(FIXED_LIT), canonical_codes(FIXED_DIST)
        self.blocks.append("fixed")
        return self

    def dynamic(self, lit_lens, dist_lens, final=False, cl_lens=None, hclen=None, items=None, hlit=None, hdist=None,
                check_items=True):
        """lit_lens / dist_lens: the code lengths of the HLIT literal/length and HDIST distance symbols (their counts are the
        header's, unless `hlit` / `hdist` name other counts for the two 5-bit fields).  items: the run-length form of the two
        lists, item by item (rle_items' format); None: rle_items.  cl_lens: the 19 lengths of the code length code by symbol;
        None: a complete code over the symbols the items use.  hclen: how many of them the header holds (4..19); None: up to
        the last one that is not zero."""
        lens = list(lit_lens) + list(dist_lens)
        if items is None:
            items = rle_items(lens)
        elif check_items:
            assert expand_items(items) == lens, "the items do not spell the lengths"
        if cl_lens is None:
            used = sorted({it[0] if isinstance(it, tuple) else it for it in items})
            if len(used) == 1:
                used.append(0 if used[0] != 0 else 1)        # (a single code would be an incomplete set)
            k = len(used).bit_length() - 1                   # 2^k <= n: 2^(k+1) - n codes of k bits, the others k + 1
            short = (2 << k) - len(used)
            cl_lens = lens_of({s: (k if i < short else k + 1) for i, s in enumerate(used)}, 19)
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        n_lit = len(lit_lens) if hlit is None else hlit
        n_dist = len(dist_lens) if hdist is None else hdist
        w = self.w
        w.bits(1 if final else 0, 1)
        w.bits(2, 2)
        w.bits(n_lit - 257, 5)
        w.bits(n_dist - 1, 5)
        w.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.bits(cl_lens[s], 3)
        cl = canonical_codes(cl_lens)
        for it in items:
            sym, n = it if isinstance(it, tuple) else (it, 0)
            w.code(*cl[sym])
            if sym == 16:
                w.bits(n - 3, 2)
            elif sym == 17:
                w.bits(n - 3, 3)
            elif sym == 18:
                w.bits(n - 11, 7)
        self.lit, self.dist = canonical_codes(lit_lens), canonical_codes(dist_lens)
        self.blocks.append("dynamic")
        return self

    # ---- symbols ----
    def bits(self, v, n):
        self.w.bits(v, n)
        return self

    def symbol(self, s):
        """One literal/length symbol's code, nothing behind it."""
        self.w.code(*self.lit[s])
        self.longest_lit = max(self.longest_lit, self.lit[s][1])
        return self

    def literal(self, b):
        self.symbol(b)
        self.out.append(b)
        return self

    def literals(self, data):
        for b in data:
            self.literal(b)
        return self

    def end_of_block(self):
        return self.symbol(END)

    def match(self, length, distance):
        ls, le = length_symbol(length)
        ds, de = distance_symbol(distance)
        return self.match_raw(ls, le, ds, de)

    def match_raw(self, len_sym, len_extra, dist_sym, dist_extra):
        """Any length symbol (257..287) with any value of its extra bits, any distance symbol (0..31) with any value of its
        extra bits: the non-canonical forms (length 258 as symbol 284 + 31) and the invalid ones."""
        self.symbol(len_sym)
        valid = len_sym <= 285 and dist_sym <= 29
        if len_sym <= 285:
            self.w.bits(len_extra, LENGTH_EXTRA[len_sym - 257])
        self.w.code(*self.dist[dist_sym])
        self.longest_dist = max(self.longest_dist, self.dist[dist_sym][1])
        if dist_sym <= 29:
            self.w.bits(dist_extra, DIST_EXTRA[dist_sym])
        if valid:
            length, distance = LENGTH_BASE[len_sym - 257] + len_extra, DIST_BASE[dist_sym] + dist_extra
            for _ in range(length):
                self.out.append(self.out[-distance] if distance <= len(self.out) else 0)
        return self


def bgzf_member(deflate_bytes, payload):
    """The member a BGZF file would hold: 18 bytes of header (the BC subfield with the member's size), the stream, the CRC-32
    and the length of `payload`."""
    bsize = 18 + len(deflate_bytes) + 8
    assert bsize <= 65536
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1) + bytes(deflate_bytes) +
            struct.pack("<II", zlib.crc32(bytes(payload)), len(payload)))


# ---------------------------------------------------------------------------------------------------------------------------
# The catalogue.  A case builds (raw DEFLATE bytes, payload).  VALID: zlib returns exactly the payload, and so must the device.
# INVALID: the payload is what the member's trailer claims (CRC-32 and ISIZE); `zlib` says how zlib answers the stream -- a
# key word of its error message, or
#   "unfinished"  the stream does not end within its bytes: eof stays false
#   "long"        the stream is sound and produces more bytes than ISIZE (limited to ISIZE bytes of output, eof stays false)
#   "short"       the stream ends having produced fewer bytes than ISIZE
#   "differs"     the stream is sound and produces other bytes than the trailer's CRC-32 covers
# and `device` is the key word of the device's status text (None: no specific one).
class Case(object):
    def __init__(self, name, fn, zlib_says=None, device=None):
        self.name, self.fn, self.zlib, self.device = name, fn, zlib_says, device
        self._built = None

    def build(self):
        if self._built is None:
            r = self.fn()
            stream, payload = (r, r.out) if isinstance(r, Deflate) else r
            if isinstance(stream, Deflate):
                stream = stream.getvalue()
            self._built = (bytes(stream), bytes(payload))
        return self._built

    def __repr__(self):
        return self.name


VALID, INVALID = [], []


def valid(name):
    def add(fn):
        VALID.append(Case(name, fn))
        return fn
    return add


def invalid(name, zlib_says, device=None):
    def add(fn):
        INVALID.append(Case(name, fn, zlib_says, device))
        return fn
    return add


A, B, C = 97, 98, 99
SMALL = {A: 1, END: 2, 257: 2}                  # 'a', end-of-block, length 3: a complete set of three codes


def _data(seed, n, lo=0, hi=256):
    return bytes(np.random.default_rng(seed).integers(lo, hi, n, dtype=np.uint8))


# ---- Huffman sets -----------------------------------------------------------------------------------------------------------
@valid("single distance code of length 1")
def _():
    d = Deflate().dynamic(lens_of(SMALL, 258), [1], final=True)
    return d.literal(A).match(3, 1).match(3, 1).end_of_block()


@valid("no distance code")
def _():
    d = Deflate().dynamic(lens_of({A: 1, B: 2, END: 2}, 257), [0], final=True)
    return d.literals(b"abba" * 20).end_of_block()


@valid("literal/length set of two codes")
def _():
    d = Deflate().dynamic(lens_of({A: 1, END: 1}, 257), [0], final=True)
    return d.literals(b"a" * 70).end_of_block()


# ---- long codes ---------------------------------------------------------------------------------------------------------------
def _long_set(deep):
    """Lengths 1, 2, ..., 14, 15, 15: thirteen literals on 1 to 13 bits, then 'z', length symbol 260 (6 bytes) and the
    end-of-block code on 14, 15 and 15 bits in the order `deep` gives."""
    spec = {ord("a") + k: k + 1 for k in range(13)}
    spec.update({deep[0]: 14, deep[1]: 15, deep[2]: 15})
    lens = lens_of(spec, 261)
    assert sorted(l for l in lens if l) == list(range(1, 15)) + [15, 15] and kraft(lens) == 32768
    return lens


def _long_code_case(deep):
    def build():
        d = Deflate().dynamic(_long_set(deep), [2, 2, 2, 2], final=True)
        d.literals(b"abcdefghijklmz").match(6, 1).literals(b"zmz").match(6, 4).match(6, 2)
        d.literals(b"aaaaaaaabbbbz" * 3).match(6, 3).literals(b"lkjihg").match(6, 1).match(6, 1)
        return d.literal(ord("z")).end_of_block()
    return build


for _name, _deep in (("literal on 14 bits, length symbol and end-of-block on 15", (122, 260, END)),
                     ("length symbol on 14 bits, end-of-block and literal on 15", (260, END, 122)),
                     ("end-of-block on 14 bits, literal and length symbol on 15", (END, 122, 260))):
    valid("long codes: " + _name)(_long_code_case(_deep))


def _sixteen(lits, lens, pad):
    """A complete literal/length set of 4-bit codes: the literals, the end-of-block code and the length symbols."""
    syms = list(lits) + [END] + list(lens) + list(pad)
    assert len(syms) == 16
    return lens_of({s: 4 for s in syms}, 286)


@valid("distance codes of 9 to 15 bits, short matches and a long one")
def _():
    lit = _sixteen(b"abcdefgh", (257, 258, 264, 269, 277, 280), (285,))
    dist = [15, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1]      # distances 1 .. 16 on 15 .. 9 bits, 17 .. 256 below
    d = Deflate().dynamic(lit, dist, final=True).literals(b"abcdefghhgfedcbaabcd")
    for length, distance in ((3, 1), (4, 2), (3, 3), (10, 4), (4, 5), (3, 7), (20, 8), (3, 9), (10, 13), (4, 16), (3, 20)):
        d.match(length, distance).literal(A + length % 8)
    d.match(80, 1).literal(B).match(120, 3).match(70, 13).literal(C).match(258, 200)
    return d.end_of_block()


# ---- lengths and distances ----------------------------------------------------------------------------------------------------
@valid("length 258 as symbol 285 and as symbol 284 with extra bits 31")
def _():
    d = Deflate().fixed(final=True).literals(b"xy").match(258, 1).literal(A).match_raw(284, 31, 1, 0).literal(B)
    return d.match_raw(284, 31, 0, 0).match(258, 2).end_of_block()


GRID_LENGTHS = (3, 4, 10, 11, 64, 65, 257, 258)
GRID_DISTANCES = (1, 2, 4, 5, 63, 64, 65, 16385, 24576, 24577, 32768)      # distance symbols 0, 1, 3, 4, 11, 12, 28, 29


@valid("length / distance grid")
def _():
    d = Deflate().stored(_data(21, 32768), final=False).fixed(final=True)
    for distance in GRID_DISTANCES:
        for length in GRID_LENGTHS:
            d.match(length, distance)
        d.literal(distance & 0xff)
    return d.end_of_block()


@valid("length / distance grid, a literal between the matches")
def _():
    d = Deflate().stored(_data(22, 32768), final=False).fixed(final=True)
    for k, length in enumerate(GRID_LENGTHS):
        for distance in GRID_DISTANCES:
            d.match(length, distance).literal((k + distance) & 0xff)
    return d.end_of_block()


def _every_length_symbol(d):
    d.literals(b"pq")
    for s in range(257, 286):
        top = (1 << LENGTH_EXTRA[s - 257]) - 1
        d.match_raw(s, 0, 1, 0).literal(s & 0xff).match_raw(s, top, 0, 0).match_raw(s, top // 2, 5, 1)
    return d.end_of_block()


@valid("every length symbol, fixed block")
def _():
    return _every_length_symbol(Deflate().fixed(final=True))


@valid("every length symbol, random complete sets of 286 and 30 codes")
def _():
    rng = np.random.default_rng(23)
    return _every_length_symbol(Deflate().dynamic(complete_lengths(rng, 286), complete_lengths(rng, 30), final=True))


# ---- a distance that reaches the first byte produced ------------------------------------------------------------------------------
def _deep_length_set():
    """'a', 'b', 'c' and the end-of-block code on 2 and 3 bits, the length symbols 257 and 285 on 12 bits."""
    return complete_with({A: 2, B: 2, C: 3, END: 3, 257: 12, 285: 12}, 286, range(100, 120))


@valid("distance = bytes produced: a 3-byte match in a small step")
def _():
    return Deflate().fixed(final=True).literals(b"abc").match(3, 3).literals(b"d").match(7, 7).end_of_block()


@valid("distance = bytes produced: matches of more than 64 bytes")
def _():
    d = Deflate().fixed(final=True).literal(A).match(100, 1).match(200, 101)
    return d.literals(_data(24, 70)).match(258, 371).end_of_block()


@valid("distance = bytes produced: a length code of 12 bits")
def _():
    d = Deflate().dynamic(_deep_length_set(), [2, 2, 2, 2], final=True)
    return d.literals(b"abc").match(3, 3).match(258, 3).literals(b"cab").end_of_block()


# ---- the dynamic header -------------------------------------------------------------------------------------------------------
@valid("HCLEN = 5: 256 codes of 8 bits")
def _():
    # (with HCLEN = 4 only the symbols 16, 17, 18 and 0 have a code: every length is zero and no such block is valid -- that
    # header is in the INVALID list; 5 adds the length 8, of which a complete set has exactly 256)
    lit = [8] * 255 + [0, 8]
    items = [8] + [(16, 6)] * 42 + [8, 8, 0, 8, 0]
    d = Deflate().dynamic(lit, [0], final=True, cl_lens=lens_of({16: 1, 0: 2, 8: 2}, 19), hclen=5, items=items)
    return d.literals(_data(25, 90, 0, 255)).end_of_block()


@valid("HCLEN field 4: eight code length code lengths")
def _():
    # lengths 7 (x 128) and 0 only: symbols 16, 17, 18, 0, 8, 7, 9, 6 are in the header
    lit = lens_of({s: 7 for s in list(range(127)) + [END]}, 257)
    d = Deflate().dynamic(lit, [0], final=True, cl_lens=lens_of({16: 2, 18: 2, 7: 2, 0: 2}, 19), hclen=8)
    return d.literals(_data(26, 90, 0, 127)).end_of_block()


@valid("HCLEN = 19: a 15-bit code in the header")
def _():
    d = Deflate().dynamic(_long_set((122, 260, END)), [1, 1], final=True, hclen=19)
    return d.literals(b"abz").match(6, 2).end_of_block()


@valid("HLIT = 257 and HDIST = 1")
def _():
    return Deflate().dynamic(lens_of({A: 1, B: 2, END: 2}, 257), [0], final=True).literals(b"abab").end_of_block()


@valid("HLIT = 286 and HDIST = 30")
def _():
    lit = lens_of({A: 1, END: 2, 285: 3, 257: 4, 0: 5, 255: 5}, 286)
    dist = lens_of({0: 1, 28: 2, 29: 2}, 30)
    d = Deflate().stored(_data(27, 24577)).dynamic(lit, dist, final=True)
    return d.literal(A).match(258, 1).match(258, 24577 + 100).literal(0).literal(255).match_raw(257, 0, 28, 0).end_of_block()


@valid("an 18 with 138 zeros")
def _():
    lit = lens_of({200: 2, 201: 2, END: 1}, 257)
    items = [(18, 138), (18, 62), 2, 2, (18, 54), 1, 0]
    assert items[0] == (18, 138)
    d = Deflate().dynamic(lit, [0], final=True, items=items)
    return d.literals(bytes([200, 201, 201, 200])).end_of_block()


@valid("a 16 that crosses from the literal/length lengths into the distance lengths")
def _():
    # symbols 255 to 258 and eight distance symbols all have 3 bits: one length, then a 16 of six more over the seam, and a 16 of five
    lit = lens_of({A: 1, 255: 3, END: 3, 257: 3, 258: 3}, 259)
    items = [(18, 97), 1, (18, 138), (18, 19), 3, (16, 6), (16, 5)]
    d = Deflate().dynamic(lit, [3] * 8, final=True, items=items)
    return d.literals(b"a\xffa").match(3, 2).match(4, 1).end_of_block()


@valid("a 16 directly after a 17 and after an 18")
def _():
    # a 16 repeats the previous LENGTH, which after a 17 or an 18 is zero
    lit = lens_of({20: 2, 40: 2, END: 1}, 257)
    items = [(17, 10), (16, 6), (16, 4), 2, (18, 11), (16, 6), 0, 0, 2, (17, 7), (16, 6), (16, 6), (16, 6), (18, 138), (18, 52), 1, 0]
    d = Deflate().dynamic(lit, [0], final=True, items=items)
    return d.literals(bytes([20, 40, 40, 20])).end_of_block()


@valid("the last run ends exactly at HLIT + HDIST")
def _():
    # an 18 that ends on the last distance length, behind the end-of-block code; the block before it ends its header with a 16
    lit = lens_of({A: 1, END: 1}, 257)
    d = Deflate().dynamic(lit, [0] * 30, items=[(18, 97), 1, (18, 138), (18, 20), 1, (18, 30)])
    d.literals(b"aa").end_of_block()
    lit = lens_of({A: 2, END: 2, 257: 2, 258: 2}, 259)
    d.dynamic(lit, [2, 2, 2, 2], final=True, items=[(18, 97), 2, (18, 138), (18, 20), 2, (16, 6)])
    return d.literal(A).match(3, 1).match(4, 4).end_of_block()


# ---- block structure ----------------------------------------------------------------------------------------------------------
@valid("a stored block at each of the 8 bit alignments")
def _():
    d = Deflate()
    seen = set()
    for k in range(8):
        # a fixed block of k 9-bit literals ends at bit 2 + k of a byte behind the stored block before it
        d.fixed().literals(bytes([144 + 13 * k + j for j in range(k)])).end_of_block()
        seen.add(d.w.nbits % 8)
        d.stored(_data(30 + k, 5 + 9 * k), final=(k == 7))
    assert seen == set(range(8))
    return d


@valid("a stored block of LEN = 0 in mid-member")
def _():
    d = Deflate().fixed().literals(b"abc").end_of_block().stored(b"").fixed().match(3, 3).end_of_block().stored(b"")
    return d.stored(b"xyz").stored(b"").fixed(final=True).match(4, 2).end_of_block()


@valid("matches that reach back into a stored block and across a dynamic block boundary")
def _():
    lit = _sixteen(b"abcdefgh", (257, 258, 264, 269, 277, 280), (285,))
    dist = complete_with({0: 2, 2: 2, 16: 2, 17: 3}, 18, [5, 9, 10])
    d = Deflate().stored(_data(40, 300)).fixed().match(10, 300).match(100, 155).literal(A).end_of_block()
    # 411 bytes so far: a dynamic block's first symbol reaches the member's first byte, through the fixed and the stored block
    d.dynamic(lit, dist).match(10, 411).match(3, 300).literals(b"hg").match(80, 3).end_of_block()
    d.dynamic(lit, dist).match(4, 1).match(120, 95 + 411).end_of_block()
    d.stored(b"0123456789").fixed(final=True).match(10, 10).match(258, 300).end_of_block()
    return d


@valid("a match as the first symbol behind a block header and as the last before end-of-block")
def _():
    d = Deflate().fixed().literals(b"ab").end_of_block()
    d.fixed().match(3, 2).end_of_block()                                        # both at once
    d.dynamic(lens_of(SMALL, 258), [1]).match(3, 1).literal(A).match(3, 1).end_of_block()
    d.fixed().match(70, 5).literal(C).match(200, 71).end_of_block()              # the long-match path on both sides
    return d.fixed(final=True).match(3, 1).end_of_block()


@valid("a final block that is an empty fixed block")
def _():
    return Deflate().stored(b"hello").fixed().literals(b" world").end_of_block().fixed(final=True).end_of_block()


@valid("four blocks of three types")
def _():
    d = Deflate().stored(b"stored first, ").fixed().literals(b"fixed, ").match(6, 7).end_of_block()
    d.dynamic(lens_of(SMALL, 258), [1]).literal(A).match(3, 1).end_of_block()
    return d.stored(b" and stored", final=True)


# ---- ISIZE ------------------------------------------------------------------------------------------------------------------------
@valid("65 280 bytes from matches")
def _():
    d = Deflate().fixed(final=True).literal(7)
    for _ in range(253):
        d.match(258, 1)
    d.match(5, 1).end_of_block()
    assert len(d.out) == 65280
    return d


@valid("65 280 bytes stored")
def _():
    return Deflate().stored(_data(41, 65280), final=True)


@valid("65 280 bytes, the last one a literal behind a long match")
def _():
    d = Deflate().stored(_data(42, 65021)).fixed(final=True).match(258, 65021 // 2).literal(1).end_of_block()
    assert len(d.out) == 65280
    return d


@valid("0 bytes: a dynamic block of the end-of-block code alone")
def _():
    return Deflate().dynamic(lens_of({0: 1, END: 1}, 257), [0], final=True).end_of_block()


@valid("0 bytes: an empty stored block, then an empty fixed block")
def _():
    return Deflate().stored(b"").fixed(final=True).end_of_block()


# ---- INVALID ------------------------------------------------------------------------------------------------------------------------
LIT_SET, DIST_SET, CL_SET = "invalid literal/lengths set", "invalid distances set", "invalid code lengths set"


@invalid("over-subscribed literal/length set", LIT_SET, "over-subscribed")
def _():
    return Deflate().dynamic(lens_of({A: 1, B: 1, END: 1}, 257), [0], final=True).literal(A).end_of_block()


@invalid("over-subscribed distance set", DIST_SET, "over-subscribed")
def _():
    return Deflate().dynamic(lens_of(SMALL, 258), [1, 1, 1], final=True).literal(A).match(3, 1).end_of_block()


@invalid("over-subscribed code length set", CL_SET, "over-subscribed")
def _():
    d = Deflate().dynamic(lens_of({A: 1, END: 1}, 257), [0], final=True, cl_lens=lens_of({0: 1, 1: 1, 18: 1, 17: 2}, 19))
    return d.literal(A).end_of_block()


@invalid("incomplete literal/length set", LIT_SET, "incomplete")
def _():
    return Deflate().dynamic(lens_of({A: 1, END: 2}, 257), [0], final=True).literals(b"aa").end_of_block()


@invalid("incomplete literal/length set with a distance set of one code", LIT_SET, "incomplete")
def _():
    d = Deflate().dynamic(lens_of({A: 2, B: 2, END: 3, 257: 3}, 258), [1], final=True)
    return d.literals(b"ab").match(3, 1).end_of_block()


@invalid("incomplete distance set of two codes", DIST_SET, "incomplete")
def _():
    return Deflate().dynamic(lens_of(SMALL, 258), [2, 2], final=True).literal(A).match(3, 1).end_of_block()


@invalid("incomplete distance set: one code of 2 bits", DIST_SET, "incomplete")
def _():
    return Deflate().dynamic(lens_of(SMALL, 258), [2], final=True).literal(A).match(3, 1).end_of_block()


@invalid("incomplete code length set", CL_SET, "incomplete")
def _():
    d = Deflate().dynamic(lens_of({A: 1, END: 1}, 257), [0], final=True, cl_lens=lens_of({0: 2, 1: 2, 18: 2}, 19))
    return d.literals(b"aaa").end_of_block()


@invalid("code length set of a single code", CL_SET, "incomplete")
def _():
    d = Deflate().dynamic([1] * 257, [1], final=True, cl_lens=lens_of({1: 1}, 19), items=[1] * 258)
    return d.bits(0, 16), b""


@invalid("no end-of-block code", "missing end-of-block", "end-of-block")
def _():
    d = Deflate().dynamic(lens_of({A: 1, B: 1}, 257), [0], final=True).literals(b"ab")
    return d.bits(0, 8), b"ab"


@invalid("HCLEN = 4: only zero lengths can be written", "missing end-of-block", "end-of-block")
def _():
    d = Deflate().dynamic([0] * 257, [0], final=True, cl_lens=lens_of({18: 1, 0: 1}, 19), hclen=4)
    return d.bits(0, 8), b""


def _counts(hlit=None, hdist=None):
    def build():
        d = Deflate().dynamic(lens_of(SMALL, 258), [1], final=True, hlit=hlit, hdist=hdist)
        return d.literal(A).match(3, 1).end_of_block()
    return build


for _k in (287, 288):
    invalid("HLIT = %d" % _k, "too many length or distance symbols", "HLIT")(_counts(hlit=_k))
for _k in (31, 32):
    invalid("HDIST = %d" % _k, "too many length or distance symbols", "HLIT")(_counts(hdist=_k))


def _repeat(items):
    def build():
        d = Deflate().dynamic(lens_of({A: 1, END: 1}, 257), [0], final=True, items=items, check_items=False,
                              cl_lens=lens_of({0: 3, 1: 3, 16: 2, 17: 2, 18: 2}, 19))
        assert kraft([3, 3, 2, 2, 2]) == 32768
        return d.bits(0, 16), b""
    return build


_HEAD = [(18, 97), 1, (18, 138), (18, 20), 1]                   # 257 lengths: one more is left
invalid("a 16 at position 0", "invalid bit length repeat", "repeat")(_repeat([(16, 3)] + _HEAD))
invalid("a 16 that runs past HLIT + HDIST", "invalid bit length repeat", "repeat")(_repeat(_HEAD + [(16, 3)]))
invalid("a 17 that runs past HLIT + HDIST", "invalid bit length repeat", "repeat")(_repeat(_HEAD + [(17, 3)]))
invalid("an 18 that runs past HLIT + HDIST", "invalid bit length repeat", "repeat")(_repeat(_HEAD[:4] + [(18, 11)]))


def _fixed_symbol(s):
    return lambda: (Deflate().fixed(final=True).literals(b"ab").symbol(s).bits(0, 16).getvalue(), b"ab")


def _fixed_distance(s):
    return lambda: (Deflate().fixed(final=True).literals(b"ab").match_raw(257, 0, s, 0).bits(0, 16).getvalue(), b"ab")


for _k in (286, 287):
    invalid("fixed block: literal/length symbol %d" % _k, "invalid literal/length code", "length symbol")(_fixed_symbol(_k))
for _k in (30, 31):
    invalid("fixed block: distance symbol %d" % _k, "invalid distance code", "no code")(_fixed_distance(_k))


@invalid("bits that are no code of a distance set of one code", "invalid distance code", "no code")
def _():
    d = Deflate().dynamic(lens_of(SMALL, 258), [1], final=True).literal(A).symbol(257)
    return d.bits(1, 1).bits(0, 16).getvalue(), b"a"


@invalid("a length symbol without any distance code", "invalid distance code", "no code")
def _():
    d = Deflate().dynamic(lens_of(SMALL, 258), [0], final=True).literal(A).symbol(257)
    return d.bits(0, 16).getvalue(), b"a"


FAR = "invalid distance too far back"


@invalid("distance = bytes produced + 1: a 3-byte match in a small step", FAR, "distance")
def _():
    return Deflate().fixed(final=True).literals(b"ab").match(3, 3).literals(b"c").end_of_block()


@invalid("distance = bytes produced + 1: a match of more than 64 bytes", FAR, "distance")
def _():
    return Deflate().fixed(final=True).literal(A).match(100, 2).literal(B).end_of_block()


@invalid("distance = bytes produced + 1: a length code of 12 bits", FAR, "distance")
def _():
    d = Deflate().dynamic(_deep_length_set(), [2, 2, 2, 2], final=True)
    return d.literals(b"ab").match(3, 3).literals(b"c").end_of_block()


@invalid("distance 1 with nothing produced: a 3-byte match", FAR, "distance")
def _():
    return Deflate().fixed(final=True).match(3, 1).literals(b"ab").end_of_block()


@invalid("distance 1 with nothing produced: a match of 100 bytes", FAR, "distance")
def _():
    return Deflate().fixed(final=True).match(100, 1).literals(b"ab").end_of_block()


@invalid("distance = bytes produced + 1 in a second block", FAR, "distance")
def _():
    return Deflate().stored(b"0123456789").fixed(final=True).literal(A).match(4, 12).end_of_block()


@invalid("output past ISIZE: a literal in a small step", "long", "ISIZE")
def _():
    d = Deflate().fixed(final=True).literals(b"abcdefg").end_of_block()
    return d.getvalue(), d.out[:-1]


@invalid("output past ISIZE: a literal on a 14-bit code", "long", "ISIZE")
def _():
    d = Deflate().dynamic(_long_set((122, 260, END)), [1, 1], final=True).literals(b"abcabcz").end_of_block()
    return d.getvalue(), d.out[:-1]


@invalid("output past ISIZE: a 258-byte match that starts 3 bytes before the end", "long", "ISIZE")
def _():
    d = Deflate().fixed(final=True).literals(b"abcdefg").match(258, 7).end_of_block()
    return d.getvalue(), d.out[:10]


@invalid("output past ISIZE: a stored block", "long", "ISIZE")
def _():
    d = Deflate().fixed().literals(b"abc").end_of_block().stored(_data(50, 100), final=True)
    return d.getvalue(), d.out[:102]


@invalid("output one byte short of ISIZE", "short", "ISIZE")
def _():
    d = Deflate().fixed(final=True).literals(b"abcdefg").match(20, 3).end_of_block()
    return d.getvalue(), bytes(d.out) + b"h"


@invalid("a sound stream under the CRC-32 of other bytes", "differs", "CRC32")
def _():
    d = Deflate().fixed(final=True).literals(b"abcdefg").match(20, 3).end_of_block()
    return d.getvalue(), bytes(d.out[:-1]) + b"h"


@invalid("comp_len one byte short: the end-of-block code lies beyond it", "unfinished", "beyond the block")
def _():
    # five 9-bit literals behind the 3 header bits: the end-of-block code (seven zero bits) is the stream's last byte.  Cut
    # off, the byte in its place is the first of the trailer's CRC-32: the payload is chosen so that it reads as that code too.
    for k in range(4096):
        d = Deflate().stored(struct.pack("<H", k)).fixed(final=True).literals(bytes([200, 201, 202, 203, 204]))
        assert d.w.nbits % 8 == 0
        d.end_of_block()
        if zlib.crc32(bytes(d.out)) & 0x7f == 0:
            return d.getvalue()[:-1], d.out
    raise AssertionError("no payload found")


@invalid("a stored block whose LEN reaches past comp_len", "unfinished", "beyond the block")
def _():
    d = Deflate().fixed().literals(b"abc").end_of_block().stored(b"0123456789", final=True, length=200)
    return d.getvalue(), b"abc" + bytes(200)


@invalid("reserved block type in a second block", "invalid block type", "reserved")
def _():
    d = Deflate().fixed().literals(b"abc").end_of_block().reserved(final=True)
    return d.bits(0, 16).getvalue(), b"abc"


@invalid("NLEN wrong in a second block", "invalid stored block lengths", "LEN")
def _():
    d = Deflate().fixed().literals(b"abc").end_of_block().stored(b"0123", final=True, nlen=0xfffa)
    return d.getvalue(), b"abc0123"


def zlib_verdict(stream, payload):
    """How zlib answers a case: (a key, the bytes it produced).  The key is zlib's error message, or "ok", "unfinished", "long",
    "short" or "differs" as the catalogue's header describes them."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream)
    except zlib.error as err:
        return str(err), b""
    if not d.eof:
        return "unfinished", out
    if out == payload and not d.unused_data:
        return "ok", out
    return ("long" if len(out) > len(payload) else "short" if len(out) < len(payload) else "differs"), out


# ---- random streams ---------------------------------------------------------------------------------------------------------------
RANDOM_SEED, RANDOM_MEMBERS, RANDOM_MAX_OUT = 20261, 256, 4096


def _random_match(rng, have, room, len_syms, dist_syms):
    """(length symbol, extra, distance symbol, extra) of a match of at most `room` bytes that reaches at most `have` bytes back,
    over the given symbols (None: any length 3..258, any distance 1..have); None where no symbol fits."""
    if len_syms is None:
        ls, le = length_symbol(int(rng.integers(3, min(258, room) + 1)))
    else:
        fit = [int(s) for s in len_syms if LENGTH_BASE[s - 257] <= room]
        if not fit:
            return None
        ls = fit[int(rng.integers(len(fit)))]
        le = int(rng.integers(min(1 << LENGTH_EXTRA[ls - 257], room - LENGTH_BASE[ls - 257] + 1)))
    near = rng.random() < 0.5
    if dist_syms is None:
        ds, de = distance_symbol(int(rng.integers(1, (min(have, 40) if near else have) + 1)))
    else:
        fit = [int(s) for s in dist_syms if DIST_BASE[s] <= have]
        if not fit:
            return None
        ds = fit[0] if near else fit[int(rng.integers(len(fit)))]
        de = int(rng.integers(min(1 << DIST_EXTRA[ds], have - DIST_BASE[ds] + 1)))
    return ls, le, ds, de


def _random_ops(rng, have, budget, alphabet, len_syms, dist_syms):
    """A random symbol sequence of at most `budget` bytes behind `have` bytes of output: (literal,) or a match's four numbers."""
    ops, made = [], 0
    for _ in range(int(rng.integers(1, 120))):
        room = budget - made
        if room <= 0:
            break
        m = None
        if have + made and room >= 3 and rng.random() < 0.45:
            m = _random_match(rng, have + made, room, len_syms, dist_syms)
        if m is None:
            ops.append((int(alphabet[int(rng.integers(len(alphabet)))]),))
            made += 1
        else:
            ops.append(m)
            made += LENGTH_BASE[m[0] - 257] + m[1]
    return ops


def random_member(rng):
    """One valid stream of 1 to 4 blocks of random type and at most RANDOM_MAX_OUT bytes of output -> Deflate.  A dynamic block's sets are complete_lengths over the literals it uses, a few length
    symbols, the end-of-block code and 1 to 30 distance symbols (one distance symbol: a single code of length 1)."""
    d = Deflate()
    n_blocks = int(rng.integers(1, 5))
    for b in range(n_blocks):
        final = b == n_blocks - 1
        budget = min(RANDOM_MAX_OUT - len(d.out), int(rng.integers(0, 2000)))
        kind = int(rng.integers(3))
        alphabet = rng.choice(256, int(rng.integers(1, 257)), replace=False)
        if kind == 0:
            d.stored(bytes(rng.integers(0, 256, min(budget, int(rng.integers(0, 600))), dtype=np.uint8)), final=final)
            continue
        if kind == 1:
            d.fixed(final=final)
            ops = _random_ops(rng, len(d.out), budget, alphabet, None, None)
        else:
            len_syms = np.sort(rng.choice(np.arange(257, 286), int(rng.integers(0, 9)), replace=False))
            dist_syms = np.sort(rng.choice(30, int(rng.integers(1, 31)), replace=False))
            ops = _random_ops(rng, len(d.out), budget, alphabet, len_syms, dist_syms)
            syms = sorted({op[0] for op in ops if len(op) == 1}) + [END] + [int(s) for s in len_syms]
            if len(syms) < 2:
                syms = [int(alphabet[0]) if alphabet[0] < 256 else 0] + syms
            lit_lens = lens_of(dict(zip(syms, complete_lengths(rng, len(syms)))), max(syms[-1] + 1, 257))
            top = int(dist_syms[-1]) + 1
            if len(dist_syms) == 1:
                dist_lens = lens_of({int(dist_syms[0]): 1}, top)
            else:
                dist_lens = lens_of(dict(zip((int(s) for s in dist_syms), complete_lengths(rng, len(dist_syms)))), top)
            d.dynamic(lit_lens, dist_lens, final=final)
        for op in ops:
            if len(op) == 1:
                d.literal(op[0])
            else:
                d.match_raw(*op)
        d.end_of_block()
    return d


def random_members(seed=RANDOM_SEED, n=RANDOM_MEMBERS):
    """The streams both tests run."""
    rng = np.random.default_rng(seed)
    return [random_member(rng) for _ in range(n)]
