"""Hand-built piles for the device reservoir sample (pepper_amd/csrc/encoder.hip: reservoir_keep_kernel behind
pa_encoder_set_sampling; the sampler's text is csrc/reservoir.h), at the edges of its own parts: the parallel regeneration of
the generator and what carries over from one regeneration to the next, pa_randint_mask at small i, the three loops of stride
256, the rank-to-pair scan over dead pairs, k = int(min(cap, rate * n)) in double, several intervals in one launch.  No GPU, no
tests: the catalogue is read by tests/test_sampling_cases_cpu.py (what every case promises, recomputed) and
tests/test_gpu_sampling_cases.py (the kernel).

The oracle is the reference's loop on numpy.random.RandomState(seed) (numpy_slots = tests/test_reservoir_cpu.py's
_numpy_slots), never the package's own sampler.  trace() states where in the generator's word stream every read draws.

A case is Case(family, name, seed, cap, rate, flank, intervals, expect): intervals = [(start, end, pattern)], fetched as
(start - flank, end + flank) with the candidate window (start, end); the pattern has one letter per (read, interval) pair of
the packer in file order -- L: a read with a base inside the fetch range, D: a pair that keeps no base (its read is aligned in
front of the range and reaches in with a trailing deletion, or deletes across all of it).  expect holds the properties the
case exists for, stated as literals: n / k per interval (k None: the interval is not sampled), what sampled() advances by,
`words` = {read: (first word, last word)} of the stream, `regens` = regenerations the sample takes.

Where the reads lie (reads_of): the pairs up to the pattern's last D start 30 .. 25 bases in front of the fetch range -- an L
there is 36 .. 40 bases and reaches 5 or more bases in, a D is 24M 20D (its last base 2 or more in front) or, every third one
where the case allows it, 24M <n>D 20M over the whole range --, the L behind them are 24 .. 40 bases spread in file order over
the range.  Reads copy a seeded reference but for sites where 45 % of the reads carry another base (so that which reads are
kept shows in candidates and images), 1 % noise, and a 2-base insert or 3-base deletion in a fifth of the longer ones."""
import collections
import zlib

import numpy as np

from test_reservoir_cpu import SEED, _numpy_slots as numpy_slots  # noqa: F401 -- the oracle

M, I, D = 0, 1, 2
MAX_READS = 12000                       # no case builds more
MT_N = 624
Case = collections.namedtuple("Case", "family name seed cap rate flank intervals expect")

_REF = "".join(np.random.default_rng(77).choice(list("ACGT"), 9000))
_SITE = np.flatnonzero(np.random.default_rng(78).random(len(_REF)) < 0.15)
_SITES = {int(p): "ACGT"[("ACGT".index(_REF[p]) + 1 + int(p) % 3) & 3] for p in _SITE}


def reference():
    return _REF


def allowed(cap, rate, n):
    """k as the variant driver's host form computes it (AlignmentSummarizer.py)."""
    return int(min(cap, rate * n))


def trace(seed, n, k):
    """-> {i: (first, last)} for every read i >= k: the indices of the first and the last 32-bit word randint(0, i + 1) took,
    counted from 0 over the whole stream of RandomState(seed).  Read off the generator's position (get_state()[2]): 624 after
    seeding, 1 after the first word of a regeneration."""
    rs = np.random.RandomState(seed)
    out, total, at = {}, 0, int(rs.get_state()[2])
    for i in range(k, n):
        rs.randint(0, i + 1)
        now = int(rs.get_state()[2])
        used = 0 if i == 0 else (now - at if now > at else MT_N - at + now)
        assert 0 < used < MT_N or i == 0
        out[i] = (total, total + used - 1)
        total, at = total + used, now
    return out


# ---- reads -----------------------------------------------------------------------------------------------------------------------
def _read(rng, pos, cigar):
    seq, at = [], pos
    for op, n in cigar:
        if op == M:
            for p in range(at, at + n):
                b = _REF[p]
                if p in _SITES and rng.random() < 0.45:
                    b = _SITES[p]
                elif rng.random() < 0.01:
                    b = "ACGT"[int(rng.integers(0, 4))]
                seq.append(b)
            at += n
        elif op == I:
            seq.extend("ACGT"[int(c)] for c in rng.integers(0, 4, n))
        else:
            at += n
    return dict(pos=int(pos), reverse=bool(rng.random() < 0.5), mapq=60, seq="".join(seq),
                qual=rng.integers(5, 40, len(seq)).astype(np.uint8), cigar=cigar)


def _live_read(rng, pos, n):
    """n read bases from pos; one in five of the longer ones with a 2-base insert or a 3-base deletion 8 bases before its end."""
    u = rng.random()
    if n >= 30 and u < 0.1:
        return _read(rng, pos, [(M, n - 10), (I, 2), (M, 8)])
    if n >= 30 and u < 0.2:
        return _read(rng, pos, [(M, n - 8), (D, 3), (M, 8)])
    return _read(rng, pos, [(M, n)])


def edge_group(rng, lo, hi, pattern, spanning):
    """The pairs of `pattern` as reads that start 30 .. 25 bases in front of lo, in file order."""
    out, dead = [], 0
    for j, ch in enumerate(pattern):
        pos = lo - 30 + (6 * j) // len(pattern)
        if ch == "L":
            out.append(_live_read(rng, pos, int(rng.integers(36, 41))))
        else:
            assert ch == "D"
            dead += 1
            if spanning and dead % 3 == 0:
                out.append(_read(rng, pos, [(M, 24), (D, hi + 11 - (pos + 24)), (M, 20)]))
            else:
                out.append(_read(rng, pos, [(M, 24), (D, 20)]))
    return out


def core_group(rng, p0, p1, n, length=(24, 40)):
    """n reads with a base inside, starting on p0 .. p1 in file order."""
    return [_live_read(rng, p0 + (j * (p1 - p0)) // max(1, n), int(rng.integers(length[0], length[1] + 1))) for j in range(n)]


def pile(rng, lo, hi, pattern, spanning=True):
    edge = pattern.rfind("D") + 1
    return edge_group(rng, lo, hi, pattern[:edge], spanning) + core_group(rng, lo - 20, hi - 40, len(pattern) - edge)


def bounds(case):
    """The fetch ranges [(lo, hi)] of the case's intervals."""
    return [(a - case.flank, b + case.flank) for a, b, _ in case.intervals]


def _many_reads(case, rng):
    """The reads of `many` (see _many below for what lies where)."""
    (l0, h0), (l1, h1), (l2, h2), (l3, h3), (l4, h4) = bounds(case)
    return (core_group(rng, l0 - 20, l1 - 80, MANY_OWN[0])                          # 0: its own reads ...
            + edge_group(rng, l1, h1, MANY_EDGE_1, False)                           # ... 1's edge group: all L in 0
            + core_group(rng, h0, l2 - 80, MANY_OWN[1])                             # 1's own
            + core_group(rng, l2 - 20, l2 - 5, MANY_SPAN, (40, 40))                 # the pile over the boundary of 1 and 2
            + core_group(rng, h1, l3 - 80, MANY_OWN[2])                             # 2's own
            + edge_group(rng, l3, h3, "D" * MANY_DEAD_3, False)                     # 3's pairs: L in 2, D in 3
            + core_group(rng, h3, h4 - 40, MANY_OWN[4]))                            # 4's own


_reads = {}


def reads_of(case):
    """-> the case's reads for bam_utils.write_bam (sorted by position, named q<i>), built once per case."""
    key = (case.family, case.name)
    if key not in _reads:
        rng = np.random.default_rng(zlib.crc32(("%s/%s" % key).encode()))
        if case.family == "many":
            reads = _many_reads(case, rng)
        else:
            reads = []
            for (lo, hi), (_a, _b, pattern) in zip(bounds(case), case.intervals):
                reads += pile(rng, lo, hi, pattern, spanning=True)
        assert all(x["pos"] <= y["pos"] for x, y in zip(reads, reads[1:])), key
        for i, r in enumerate(reads):
            r["name"] = "q%d" % i
        _reads[key] = reads
    return _reads[key]


def pairs_of(reads, lo, hi):
    """The packer's rule and the clip's, restated (csrc/pack_rule.h; bam_utils.restated_get_reads): -> [(read index, live)] of the
    fetch range lo .. hi in file order.  A record at pos over ref_len reference bases is a pair when pos < hi and
    pos + max(1, ref_len) > lo; it is a read of the interval when one of its aligned bases lies on lo .. hi."""
    out = []
    for idx, r in enumerate(reads):
        at, live = r["pos"], False
        for op, n in r["cigar"]:
            if op == M and at <= hi and at + n - 1 >= lo:
                live = True
            if op != I:
                at += n
        if r["pos"] < hi and max(at, r["pos"] + 1) > lo:
            out.append((idx, live))
    return out


def pattern_of(reads, lo, hi):
    return "".join("L" if live else "D" for _idx, live in pairs_of(reads, lo, hi))


def kept_reads(case, r):
    """The reads of interval r the oracle keeps (all of them where the interval is not sampled), in file order."""
    reads = reads_of(case)
    lo, hi = bounds(case)[r]
    live = [idx for idx, alive in pairs_of(reads, lo, hi) if alive]
    k = allowed(case.cap, case.rate, len(live))
    if len(live) > k:
        live = [live[s] for s in sorted(numpy_slots(case.seed, len(live), k).tolist())]
    return [reads[idx] for idx in live]


# ---- the cases -------------------------------------------------------------------------------------------------------------------
LO, HI = 1000, 1600                     # the interval of the one-interval cases
FRONT = (400, 700, "LLL")               # an interval in front of it: 3 pairs, never sampled (pair0 = 3 for the one behind it)
CASES = []


def _case(family, name, seed, cap, rate, intervals, flank=0, **expect):
    n = [p.count("L") for _a, _b, p in intervals]
    assert sum(len(p) for _a, _b, p in intervals) <= MAX_READS
    expect.setdefault("n", n)
    k = expect["k"]
    expect["sampled"] = (sum(1 for kk in k if kk is not None), sum(nn - kk for nn, kk in zip(n, k) if kk is not None))
    CASES.append(Case(family, name, seed, cap, rate, flank, list(intervals), expect))


def _one(family, name, seed, cap, rate, n, k, **expect):
    """One interval of n reads and nothing else: k = the slots it is sampled down to, None: not sampled."""
    _case(family, name, seed, cap, rate, [(LO, HI, "L" * n)], k=[k], **expect)


# regen_boundary: a sample that ends exactly on the last word of a regeneration, the read behind it, reads whose rejected words
# close a regeneration
_one("regen_boundary", "k1_ends_on_623", SEED, 1, 1.0, 419, 1, words={418: (623, 623)}, regens=1)
_one("regen_boundary", "k1_opens_second", SEED, 1, 1.0, 420, 1, words={418: (623, 623), 419: (624, 624)}, regens=2)
_one("regen_boundary", "k1_ends_on_1247", SEED, 1, 1.0, 867, 1, words={866: (1247, 1247)}, regens=2)
_one("regen_boundary", "k1_opens_third", SEED, 1, 1.0, 868, 1, words={866: (1247, 1247), 867: (1248, 1248)}, regens=3)
_one("regen_boundary", "k255_in_front_of_the_straddle", SEED, 255, 1.0, 653, 255, words={652: (621, 621)}, regens=1)
_one("regen_boundary", "k255_two_rejections_close", SEED, 255, 1.0, 654, 255, words={653: (622, 624)}, regens=2)
_one("regen_boundary", "seed5489_straddle", 5489, 1, 1.0, 419, 1, words={418: (623, 624)}, regens=2)
_one("regen_boundary", "seed5489_behind_the_straddle", 5489, 1, 1.0, 420, 1, words={418: (623, 624), 419: (625, 625)}, regens=2)
_one("regen_boundary", "seedffffffff_k64_straddle", 0xffffffff, 64, 1.0, 518, 64, words={517: (623, 624)}, regens=2)
_one("regen_boundary", "seed0_k255_four_words", 0, 255, 1.0, 1135, 255, words={1134: (1247, 1250)}, regens=3)

_one("regen_boundary", "seed1_k7_ends_on_623", 1, 7, 1.0, 449, 7, words={448: (623, 623)}, regens=1)
_one("regen_boundary", "seed1_k7_opens_second", 1, 7, 1.0, 450, 7, words={448: (623, 623), 449: (624, 624)}, regens=2)
_one("regen_boundary", "seed1_k64_three_rejections_close", 1, 64, 1.0, 523, 64, words={522: (621, 624)}, regens=2)

# mask: i = 2^b - 1 rejects nothing, i = 2^b half of the words
for _k, _n in ((1, 2), (1, 3), (1, 4), (1, 5), (2, 3), (2, 4)):
    _one("mask", "k%d_n%d" % (_k, _n), SEED, _k, 1.0, _n, _k)
_one("mask", "k3_every_power_of_two", SEED, 3, 1.0, 4100, 3, powers=tuple(1 << b for b in range(2, 13)), regens=9)

# stride: the loops of 256 over k and over n
for _k in (255, 256, 257):
    _one("stride", "k%d_n_k_plus_1" % _k, SEED, _k, 1.0, _k + 1, _k)
    _one("stride", "k%d_n_2k_plus_3" % _k, SEED, _k, 1.0, 2 * _k + 3, _k)
for _n in (255, 256, 257, 511, 512, 513):
    _one("stride", "k7_n%d" % _n, SEED, 7, 1.0, _n, 7)

# cap_edge: the largest cap
_one("cap_edge", "n5000", SEED, 5000, 1.0, 5000, None)
_one("cap_edge", "n5001", SEED, 5000, 1.0, 5001, 5000, words={5000: (0, 0)}, regens=1)
_one("cap_edge", "n10003", SEED, 5000, 1.0, 10003, 5000)
# ... and n == k / n == k + 1 with dead pairs beside the reads, so that the interval is handed to the kernel (pairs > cap)
_case("cap_edge", "n_equals_cap_among_dead_pairs", SEED, 64, 1.0, [(LO, HI, "DLD" + "L" * 63)], k=[None])
_case("cap_edge", "n_one_above_cap_among_dead_pairs", SEED, 64, 1.0, [(LO, HI, "DLD" + "L" * 64)], k=[64])

# rate: k = int(min(cap, rate * n)), one double multiply truncated toward zero
_one("rate", "half_of_1", SEED, 5000, 0.5, 1, 0)
_one("rate", "half_of_2", SEED, 5000, 0.5, 2, 1)
_one("rate", "half_of_3", SEED, 5000, 0.5, 3, 1)
_one("rate", "p29_of_100", SEED, 5000, 0.29, 100, 28)             # 0.29 * 100 = 28.999999999999996
_one("rate", "p57_of_100", SEED, 5000, 0.57, 100, 56)             # 0.57 * 100 = 56.99999999999999
_one("rate", "a_hundredth_of_60", SEED, 5000, 0.01, 60, 0)       # k = 0: the interval is emptied
_one("rate", "p999_of_1000", SEED, 5000, 0.999, 1000, 999)
_one("rate", "p999_of_1001", SEED, 5000, 0.999, 1001, 999)
_one("rate", "one_and_a_half_the_cap_decides", SEED, 100, 1.5, 161, 100)
_one("rate", "one_and_a_half_below_the_cap", SEED, 100, 1.5, 100, None)
_case("rate", "half_of_nothing", SEED, 5000, 0.5, [(LO, HI, "D" * 9)], k=[None])
_case("rate", "half_of_2_among_dead_pairs", SEED, 5000, 0.5, [(LO, HI, "DDLDLD")], k=[1])

# ranks: k = 5 of ~300 reads among ~800 pairs; dead pairs where the passes of 256 begin and end
RANK_PATTERNS = collections.OrderedDict([
    ("dead_first", "D" + "L" * 300),
    ("dead_on_255_256_257", "L" * 255 + "DDD" + "L" * 45),
    ("dead_pass", "L" * 200 + "D" * 330 + "L" * 100),                                        # pairs 200 .. 529 dead: the pass 256 .. 511 whole
    ("dead_last", "L" * 150 + "D" * 349 + "L" * 150 + "D"),
    ("alternating", "LD" * 300),
    ("alternating_dead_first", "DL" * 257 + "D" * 270 + "L" * 16),                            # 800 pairs, the last pass of 32
])
for _name, _pattern in RANK_PATTERNS.items():
    _case("ranks", _name, SEED, 5, 1.0, [(LO, HI, _pattern)], k=[5])
    _case("ranks", _name + "_second_interval", SEED, 5, 1.0, [FRONT, (LO, HI, _pattern)], k=[None, 5])
# ... and one with 40 slots, whose kept reads pile up deep enough for candidates (the downstream comparison)
_case("ranks", "alternating_dead_first_k40_second_interval", SEED, 40, 1.0, [FRONT, (LO, HI, RANK_PATTERNS["alternating_dead_first"])],
      k=[None, 40])

# many: five abutting intervals of 400 bases fetched with 50 more on either side, cap 48, rate 1.0, in one call
#   0  fewer reads than the cap: 30 of its own and the 8 of interval 1's edge group, whose aligned bases all lie in 0
#   1  sampled, dead pairs inside: the edge group LDLDDLLD, 40 of its own, the 40 of the pile over its boundary with 2
#   2  sampled: the same pile, 30 of its own, and the 50 reads whose trailing deletions are all that interval 3 sees
#   3  all D: 50 pairs (more than the cap, so the kernel gets it), no read
#   4  n == cap: 48 reads, 48 pairs
MANY_OWN, MANY_EDGE_1, MANY_SPAN, MANY_DEAD_3 = (30, 40, 30, 0, 48), "LDLDDLLD", 40, 50
_case("many", "five_abutting", SEED, 48, 1.0, flank=50, intervals=[
    (1000, 1400, "L" * 38),
    (1400, 1800, MANY_EDGE_1 + "L" * 80),
    (1800, 2200, "L" * 120),
    (2200, 2600, "D" * 50),
    (2600, 3000, "L" * 48)], k=[None, 48, 48, None, None])

FAMILIES = ("regen_boundary", "mask", "stride", "cap_edge", "rate", "ranks", "many")
DOWNSTREAM_VARIANT = (("regen_boundary", "k255_two_rejections_close"), ("ranks", "alternating_dead_first_k40_second_interval"),
                      ("many", "five_abutting"),
                      ("rate", "a_hundredth_of_60"))
DOWNSTREAM_POLISH = (("ranks", "dead_on_255_256_257"), ("regen_boundary", "k1_opens_second"))


def case(family, name):
    return next(c for c in CASES if (c.family, c.name) == (family, name))


def case_ids():
    return ["%s-%s" % (c.family, c.name) for c in CASES]
