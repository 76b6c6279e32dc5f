"""Hand-built reads for the read re-aligner (pepper_amd/csrc/realign.hip), at the edges of its bookkeeping: the 8-bit to 16-bit
switch (a running maximum of 249), the register-strip ladder of the score pass (2 .. 24 rows per lane, the LDS form beyond 1 536
padded rows), the band stage's first rows of 129 / 257 slots, its 64-cell chunks, the doubling of the half width from 1 (the
kernel's own ST_WIDER verdict past 64), stride = min(2 bw + 1, n), window ends, the longest read (MAX_READ = 4 000) and the one
stated limit of the band stage.  No GPU, no tests: the catalogue is read by tests/test_realign_cases_cpu.py (the restatement
against the reference's SSW build, the goldens, what every case promises), tests/test_gpu_realign_cases.py (the kernels) and
tests/golden/make_golden_realign_cases.py.

Every family is a function -> {name: (window_start, window_text, read_pos, read_seq, expect)}; the read is aligned against the
window's suffix that starts at read_pos, and the cases of a family share one window.  `expect` holds the properties the case
exists for (checked on the restatement's own result by the CPU module, so a case that stops hitting its edge fails there):
    score     the alignment score
    wide      the flag oracle.ssw.align returns: the 8-bit pass overflowed, the 16-bit segmentation decided
    gaps      the I / D operations of the CIGAR, in order, as (BAM code, length)
    bw        |n2 - m2| + 1 of the aligned spans: the band stage's first half width
    strip     ceil(ceil(m / 16) * 16 / 64): rows per lane of the score pass's register strip
    lds_form  more than 1 536 padded rows: the score pass keeps its column in LDS
    cigar     the whole CIGAR text
Nothing is drawn at random and nothing comes from numpy.random: base text is a splitmix64 step indexed by (salt, position), so
the inputs are the same under every numpy, and the text is not low-complexity: the planted alignment is the optimal one."""
import hashlib

MASK = (1 << 64) - 1
I, D = 1, 2                                    # BAM codes, as oracle.ssw.parse_cigar returns them


def _mix(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def text(salt, n):
    """n bases of the stream `salt`."""
    s = _mix(salt)
    return "".join("ACGT"[_mix(s + i) >> 62] for i in range(n))


def other(base, k=0):
    """A base that is not `base` (one of the three, by k)."""
    return "ACGT"[("ACGT".index(base) + 1 + k % 3) & 3]


def plant(window, at, shape, salt=0):
    """A read built along window[at:] -> (read text, BAM CIGAR with M / I / D, window bases spanned).  shape: ('=', n) copies n
    window bases, ('X', n) replaces each of n by another base, ('I', n) puts n foreign bases in (the first differs from the window
    base that follows, the last from the one before: the gap cannot slide), ('D', n) leaves n window bases out, ('R', (a, b))
    puts a bases that each differ from the window base under them in the place of b window bases."""
    seq, cigar, j = [], [], at

    def op(code, n):
        if cigar and cigar[-1][0] == code:
            cigar[-1] = (code, cigar[-1][1] + n)
        elif n:
            cigar.append((code, n))
    for k, (kind, n) in enumerate(shape):
        if kind == "=":
            seq.append(window[j:j + n])
            assert len(seq[-1]) == n, (at, shape)
            j += n
            op(0, n)
        elif kind == "X":
            seq.append("".join(other(window[j + i], salt + i) for i in range(n)))
            j += n
            op(0, n)
        elif kind == "I":
            ins = list(text(1000 + salt + 17 * k, n))
            after, before = window[j:j + 1], window[j - 1:j] if j > 0 else ""
            if ins[0] == after:
                ins[0] = next(b for b in "ACGT" if b != after and (n > 1 or b != before))
            if ins[-1] == before:
                ins[-1] = next(b for b in "TGCA" if b != before and (n > 1 or b != after))
            seq.append("".join(ins))
            op(I, n)
        elif kind == "D":
            j += n
            op(D, n)
        elif kind == "R":
            a, b = n
            seq.append("".join(other(window[j + min(i, b - 1)], salt + i) for i in range(a)))
            j += b
            op(0, min(a, b))
            op(I if a > b else D, abs(a - b))
        else:
            raise ValueError(kind)
    return "".join(seq), cigar, j - at


def strip_of(m):
    return -(-(-(-m // 16) * 16) // 64)


def _case(start, window, off, shape, salt=0, **expect):
    seq, _, _ = plant(window, off, shape, salt)
    return (start, window, start + off, seq, expect)


# ---- switch -------------------------------------------------------------------------------------------------------------------
# (name, shape, score, wide, gaps): match 4, mismatch -6, a gap of k 8 + 2 (k - 1).  Scores are even; the 8-bit pass overflows at a
# running maximum of 249, so 248 is the last narrow score and 250 the first wide one.
SWITCH_SHAPES = (
    ("copy60", [("=", 60)], 240, 0, []),
    ("copy61", [("=", 61)], 244, 0, []),
    ("copy62", [("=", 62)], 248, 0, []),
    ("copy63", [("=", 63)], 252, 1, []),
    ("copy64", [("=", 64)], 256, 1, []),
    ("sub64", [("=", 32), ("X", 1), ("=", 31)], 246, 0, []),                   # 63 matches, one mismatch
    ("sub65", [("=", 32), ("X", 1), ("=", 32)], 250, 1, []),                   # 32=1X32=: the first wide score
    ("del63", [("=", 40), ("D", 1), ("=", 23)], 244, 0, [(D, 1)]),
    ("del64", [("=", 40), ("D", 1), ("=", 24)], 248, 0, [(D, 1)]),             # the last narrow score, with a gap
    ("del65", [("=", 40), ("D", 1), ("=", 25)], 252, 1, [(D, 1)]),             # 40=1D25=
    ("ins63", [("=", 30), ("I", 1), ("=", 33)], 244, 0, [(I, 1)]),
    ("ins64", [("=", 30), ("I", 1), ("=", 34)], 248, 0, [(I, 1)]),
    ("ins66", [("=", 30), ("I", 1), ("=", 36)], 256, 1, [(I, 1)]),
)


def switch():
    start, window = 2_000, text(11, 260)
    return {name: _case(start, window, 5 + 11 * k, shape, salt=k, score=score, wide=wide, gaps=gaps)
            for k, (name, shape, score, wide, gaps) in enumerate(SWITCH_SHAPES)}


# ---- ladder -------------------------------------------------------------------------------------------------------------------
LADDER_LENGTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65) + tuple(128 * k + d for k in range(1, 13) for d in (-1, 0, 1))


def ladder_rows(m):
    """The last row of the third segment of the 16-bit (8 segments) and of the 8-bit (16 segments) layout."""
    return (("seg8", 3 * -(-m // 8) - 1), ("seg16", 3 * -(-m // 16) - 1))


def ladder():
    """Every length as an exact copy and -- where it fits -- as a copy in which three foreign bases stand for two window bases
    from the last row of the third segment on: I, D and X next to a segment start, where the library's segment-local gap chain
    differs from the exact one.  128 k - 1 and 128 k take 2 k rows per lane, 128 k + 1 takes 2 k + 1; 1 537 bases are 1 552
    padded rows: the first read of the LDS form."""
    start, window = 10_000, text(12, 1_700)
    cases = {}
    for k, m in enumerate(LADDER_LENGTHS):
        off = 3 + k % 7
        rows = -(-m // 16) * 16
        expect = dict(strip=-(-rows // 64), lds_form=rows > 1536)
        cases["copy%d" % m] = _case(start, window, off, [("=", m)], score=4 * m, wide=int(4 * m >= 249), gaps=[], cigar="%d=" % m, **expect)
        for tag, row in ladder_rows(m):
            if row >= 1 and row + 3 < m:
                cases["%s_%d" % (tag, m)] = _case(start, window, off, [("=", row), ("R", (3, 2)), ("=", m - row - 3)], salt=k, **expect)
    return cases


# ---- band_single ----------------------------------------------------------------------------------------------------------------
BAND_GAPS = (31, 32, 33, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 254, 255, 256, 257, 258)


def band_single_shapes():
    """(name, shape, gaps, bw): flanks of 300 around one deletion / one insertion of g bases: half width g + 1 at the first
    attempt.  g = 64 is the widest that the 129-slot first rows hold, 128 the widest for 257 slots; 2 g + 1 slots are 64-cell
    chunks with 1, 2, 3 ... cells in the last one."""
    out = []
    for g in BAND_GAPS:
        out.append(("del%d" % g, [("=", 300), ("D", g), ("=", 300)], [(D, g)], g + 1))
        out.append(("ins%d" % g, [("=", 300), ("I", g), ("=", 300)], [(I, g)], g + 1))
    return out


def band_single():
    start, window = 20_000, text(13, 900)
    return {name: _case(start, window, k % 5, shape, salt=k, gaps=gaps, bw=bw, wide=1)
            for k, (name, shape, gaps, bw) in enumerate(band_single_shapes())}


# ---- band_doubling --------------------------------------------------------------------------------------------------------------
DOUBLING_GAPS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 127, 128, 129)


def band_doubling_shapes():
    """300= L I 250= L D 300=: both spans are 850 + L, so the half width starts at 1 and doubles until it holds the gap.  From
    L = 65 on the first rows are too narrow and the kernel itself asks for full rows (ST_WIDER with the width it needs)."""
    return [("both%d" % L, [("=", 300), ("I", L), ("=", 250), ("D", L), ("=", 300)], [(I, L), (D, L)], 1) for L in DOUBLING_GAPS]


def band_doubling():
    start, window = 30_000, text(14, 1_000)
    return {name: _case(start, window, k % 4, shape, salt=k, gaps=gaps, bw=bw, wide=1)
            for k, (name, shape, gaps, bw) in enumerate(band_doubling_shapes())}


# ---- band_wider_than_matrix -----------------------------------------------------------------------------------------------------
def band_wider_than_matrix():
    """Flanks of 60 around an insertion of g: n2 = 120 and 2 bw + 1 = 2 g + 3 runs from 115 to 127, so stride = min(2 bw + 1, n)
    takes its other branch between g = 58 and g = 59."""
    start, window = 40_000, text(15, 300)
    return {"ins%d" % g: _case(start, window, 7 * k, [("=", 60), ("I", g), ("=", 60)], salt=k, gaps=[(I, g)], bw=g + 1, wide=1,
                               score=480 - 8 - 2 * (g - 1), cigar="60=%dI60=" % g)
            for k, g in enumerate(range(56, 63))}


# ---- window_edges ---------------------------------------------------------------------------------------------------------------
def window_edges():
    """A 40-base read against the last 1, 2, 15, 16 and 17 bases of the window (n < m); reads whose alignment ends on the window's
    last base; reads that begin with five copies of a 3-base unit the window repeats twenty times (the reversed pass finds many
    begin cells of equal score)."""
    start = 50_000
    head, tail = text(16, 300), text(17, 240)
    unit = other(tail[0]) + other(tail[0], 1) + other(tail[0], 2)         # (three different bases, none of them the base that follows)
    window = head + unit * 20 + tail
    W = len(window)
    cases = {}
    for k, n in enumerate((1, 2, 15, 16, 17)):
        seq = window[W - n:] + "".join(other(window[W - 1 - i % 7], k + i) for i in range(40 - n))
        cases["suffix%d" % n] = (start, window, start + W - n, seq, dict(score=4 * n, wide=0, gaps=[], cigar="%d=%dS" % (n, 40 - n)))
    cases["ends_on_last"] = _case(start, window, W - 80, [("=", 80)], score=320, wide=1, gaps=[], cigar="80=")
    cases["runs_past_last"] = (start, window, start + W - 70, window[W - 70:] + "ACGTACGTAC", dict(score=280, wide=1, gaps=[], cigar="70=10S"))
    at = len(head)
    cases["repeat_from_its_start"] = (start, window, start + at, unit * 5 + tail[:50], dict(score=4 * 65, wide=1, gaps=[], cigar="65="))
    cases["repeat_from_before"] = (start, window, start + at - 20, unit * 5 + tail[:50], dict(score=4 * 65, wide=1, gaps=[], cigar="65="))
    return cases


# ---- longest --------------------------------------------------------------------------------------------------------------------
def longest():
    """MAX_READ = 4 000: the cell fields are 14 bits wide (4 m < 16 384), 16 000 is the largest score the design admits.  The
    reads with a deletion are the ones whose full band rows do not fit three wavefronts' LDS (12 * 3 * (n2 + 4) + n2 + m2 + 80
    bytes > 150 KiB from n2 = 4 064 on): they take the one-wavefront band kernel.  3 000 bases with a 200-base deletion need 122 KB
    for three wavefronts: above the 64 KiB a launch gets without asking, below the limit."""
    start, window = 60_000, text(18, 4_200)
    return {
        "copy3999": _case(start, window, 100, [("=", 3999)], score=15_996, wide=1, gaps=[], cigar="3999=", strip=63, lds_form=True),
        "copy4000": _case(start, window, 100, [("=", 4000)], score=16_000, wide=1, gaps=[], cigar="4000=", strip=63, lds_form=True),
        "del64": _case(start, window, 0, [("=", 2000), ("D", 64), ("=", 2000)], score=15_866, wide=1, gaps=[(D, 64)], bw=65),
        "del200": _case(start, window, 0, [("=", 2000), ("D", 200), ("=", 2000)], score=15_594, wide=1, gaps=[(D, 200)], bw=201),
        "del200_of_3000": _case(start, window, 50, [("=", 1500), ("D", 200), ("=", 1500)], score=11_594, wide=1, gaps=[(D, 200)], bw=201),
    }


# ---- band_limit -----------------------------------------------------------------------------------------------------------------
BAND_LDS_LIMIT = 150 * 1024


def band_lds_bytes(n2, m2, waves):
    """LDS of a band round with full rows (band_rounds_host): three int arrays of n2 + 4 slots per wavefront, the two base-code
    windows, the result slots."""
    return 12 * waves * (n2 + 4) + (n2 + m2 + 16) + 64


def band_limit():
    """The one limit the band stage has beyond MAX_READ (include/pepper_amd_realign.h): 13 n2 + m2 + 128 <= 153 600 bytes with
    one wavefront per read.  Forty stretches of 100 bases with g window bases left out between them, the left-out stretches all
    N (they match nothing, so no other path competes): joining costs 6 + 2 g of the 400 a stretch scores.  g = 190: n2 = 11 410,
    152 458 bytes: aligned.  g = 194: n2 = 11 566, 154 486 bytes: refused."""
    start = 70_000
    stretches = text(19, 4_000)
    cases = {}
    for name, g in (("under", 190), ("over", 194)):
        window = ("N" * g).join(stretches[100 * k:100 * k + 100] for k in range(40)) + text(20, 30)
        n2 = 4_000 + 39 * g
        cases[name] = (start, window, start, stretches, dict(score=16_000 - 39 * (6 + 2 * g), wide=1, gaps=[(D, g)] * 39, bw=39 * g + 1,
                                                            cigar=("%dD" % g).join(["100="] * 40), n2=n2,
                                                            fits=band_lds_bytes(n2, 4_000, 1) <= BAND_LDS_LIMIT))
    return cases


FAMILIES = dict(switch=switch, ladder=ladder, band_single=band_single, band_doubling=band_doubling,
                band_wider_than_matrix=band_wider_than_matrix, window_edges=window_edges, longest=longest, band_limit=band_limit)


def window_of(cases):
    """(window_start, window_text) of a family: one window for all its cases."""
    windows = {(c[0], c[1]) for c in cases.values()}
    assert len(windows) == 1
    return next(iter(windows))


def split_by_window(cases):
    """The cases grouped by window, in order (band_limit has one window per case)."""
    out = {}
    for name, c in cases.items():
        out.setdefault((c[0], c[1]), {})[name] = c
    return list(out.values())


def input_digest(families=None):
    """SHA-256 over every family's window starts, windows, read positions and reads: the goldens hold results only, this ties
    them to the inputs they were computed from."""
    h = hashlib.sha256()
    for fam in sorted(FAMILIES):
        cases = families[fam] if families else FAMILIES[fam]()
        for name in sorted(cases):
            start, window, pos, seq, _ = cases[name]
            h.update(("%s/%s/%d/%s/%d/%s\n" % (fam, name, start, window, pos, seq)).encode())
    return h.hexdigest()
