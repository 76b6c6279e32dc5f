"""What tests/sampling_cases.py promises, recomputed without a GPU: every case's pairs are the planned pattern under the
packer's and the clip's rules restated, n and k are what the catalogue states and k is int(min(cap, rate * n)), the word-stream
edges (`words`, `regens`, the rejections at powers of two) are where trace() finds them under the installed NumPy -- and where
a second derivation from the generator's raw words finds them --, and the host build of csrc/reservoir.h
(_lib.reservoir_sample) gives the oracle's slots on every sampled interval of the catalogue."""
import numpy as np
import pytest

import sampling_cases as sc


def _want_k(case, n):
    k = sc.allowed(case.cap, case.rate, n)
    return k if n > k else None


def _raw_trace(seed, n, k):
    """trace() again from the raw 32-bit words (randint over the whole uint32 range hands them out one by one): read i takes
    words until one `& mask` is <= i, mask = the smallest 2^b - 1 >= i.  -> ({i: (first, last)}, slots)."""
    words = np.random.RandomState(seed).randint(0, 1 << 32, 2 * (n - k) + 4096, dtype=np.uint32).tolist()
    out, slots, at = {}, list(range(k)), 0
    for i in range(k, n):
        mask, first = (1 << int(i).bit_length()) - 1, at
        while True:
            v = words[at] & mask
            at += 1
            if v <= i:
                break
        if v < k:
            slots[v] = i
        out[i] = (first, at - 1)
    return out, slots


def test_the_catalogue_covers_every_family_within_its_bound():
    assert {c.family for c in sc.CASES} == set(sc.FAMILIES)
    assert len({(c.family, c.name) for c in sc.CASES}) == len(sc.CASES)
    for c in sc.CASES:
        assert 0 < len(sc.reads_of(c)) <= sc.MAX_READS, c.name
        assert 1 <= c.cap <= 5000 and c.rate >= 0
    for key in sc.DOWNSTREAM_VARIANT + sc.DOWNSTREAM_POLISH:
        sc.case(*key)
    assert {f for f, _ in sc.DOWNSTREAM_VARIANT} >= {"regen_boundary", "ranks", "many"}
    assert any(sc.case(*key).expect["k"] == [0] for key in sc.DOWNSTREAM_VARIANT)
    assert {f for f, _ in sc.DOWNSTREAM_POLISH} == {"regen_boundary", "ranks"}


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_ids())
def test_a_case_is_what_it_says(case):
    from pepper_amd import _lib
    reads, e = sc.reads_of(case), case.expect
    assert all(24 <= len(r["seq"]) <= 44 and len(r["seq"]) == len(r["qual"]) for r in reads)
    sampled = dropped = 0
    for r, ((lo, hi), (_a, _b, pattern)) in enumerate(zip(sc.bounds(case), case.intervals)):
        assert sc.pattern_of(reads, lo, hi) == pattern, (case.name, r)
        n = pattern.count("L")
        assert e["n"][r] == n and e["k"][r] == _want_k(case, n), (case.name, r, n)
        kept = sc.kept_reads(case, r)
        if e["k"][r] is None:
            assert len(kept) == n
            continue
        k = e["k"][r]
        sampled, dropped = sampled + 1, dropped + n - k
        want = sc.numpy_slots(case.seed, n, k)
        assert np.array_equal(_lib.reservoir_sample(case.seed, n, k), want)
        assert len(kept) == k == len(set(want.tolist()))
    assert e["sampled"] == (sampled, dropped)
    # every pair is a read of the file once per interval it belongs to, and the call's pairs are the patterns laid end to end
    assert sum(len(sc.pairs_of(reads, lo, hi)) for lo, hi in sc.bounds(case)) == sum(len(p) for _a, _b, p in case.intervals)


@pytest.mark.parametrize("case", [c for c in sc.CASES if "words" in c.expect or "regens" in c.expect],
                         ids=lambda c: "%s-%s" % (c.family, c.name))
def test_the_word_stream_edges_are_where_the_catalogue_puts_them(case):
    n, k = case.expect["n"][0], case.expect["k"][0]
    got = sc.trace(case.seed, n, k)
    raw, slots = _raw_trace(case.seed, n, k)
    assert got == raw and slots == sc.numpy_slots(case.seed, n, k).tolist()
    assert sorted(got) == list(range(k, n)) and got[k][0] == 0
    assert all(got[i + 1][0] == got[i][1] + 1 for i in range(k, n - 1))
    for i, span in case.expect.get("words", {}).items():
        assert got[i] == span, (i, got[i])
    assert got[n - 1][1] // sc.MT_N + 1 == case.expect["regens"]
    if "powers" in case.expect:
        # i = 2^b: the mask is 2^(b + 1) - 1, half of the words are rejected -- at least one such read did draw twice;
        # i = 2^b - 1: the mask is i itself, no word can be rejected
        powers = [p for p in case.expect["powers"] if k <= p < n]
        assert len(powers) == len(case.expect["powers"]) and max(powers) == 4096
        assert any(got[p][1] > got[p][0] for p in powers)
        assert all(got[p - 1][1] == got[p - 1][0] for p in powers if p - 1 >= k)


def test_regen_boundary_has_both_kinds_for_each_of_its_seeds():
    exact, straddle = set(), set()
    for c in sc.CASES:
        if c.family != "regen_boundary":
            continue
        n = c.expect["n"][0]
        first, last = c.expect["words"][n - 1] if n - 1 in c.expect["words"] else (None, None)
        if last is not None and last % sc.MT_N == sc.MT_N - 1 and first == last:
            exact.add(c.seed)                          # the sample ends with the last word of a regeneration
        if any(a // sc.MT_N != b // sc.MT_N for a, b in c.expect["words"].values()):
            straddle.add(c.seed)                       # rejected words end a regeneration, the accepted one opens the next
    assert {sc.SEED, 1} <= exact and {sc.SEED, 5489, 0xffffffff, 0, 1} <= straddle


def test_the_rate_cases_separate_double_from_float():
    """0.29 * 100 and 0.57 * 100 fall just short of 29 and 57 in double; one float multiply, or a rounding conversion, gives
    the integer above -- a k the catalogue's cases would show as one read too many."""
    for name, rate, k in (("p29_of_100", 0.29, 28), ("p57_of_100", 0.57, 56)):
        c = sc.case("rate", name)
        assert c.rate == rate and c.expect["k"] == [k] and rate * 100 < k + 1
        assert int(np.float32(rate) * np.float32(100)) == k + 1 and round(rate * 100) == k + 1
    assert sc.case("rate", "half_of_1").expect["k"] == [0]
    assert sc.case("rate", "half_of_nothing").expect["n"] == [0]
    c = sc.case("rate", "one_and_a_half_the_cap_decides")
    assert c.rate * c.expect["n"][0] > c.cap == c.expect["k"][0]


def test_ranks_put_dead_pairs_on_the_pass_edges():
    p = sc.RANK_PATTERNS
    assert p["dead_first"][0] == "D" and p["dead_last"][-1] == "D"
    assert p["dead_on_255_256_257"][254:259] == "LDDDL"
    assert set(p["dead_pass"][256:512]) == {"D"} and p["dead_pass"][199] == "L" and p["dead_pass"][530] == "L"
    assert p["alternating"][:4] == "LDLD" and p["alternating_dead_first"][:4] == "DLDL"
    assert all(len(q) > 256 for q in p.values()) and len(p["alternating_dead_first"]) % 256 == 32
    for name in p:
        alone, second = sc.case("ranks", name), sc.case("ranks", name + "_second_interval")
        assert alone.intervals[0][2] == second.intervals[1][2] == p[name]
        assert 0 < len(second.intervals[0][2]) <= second.cap and len(second.intervals[0][2]) % 2 == 1     # pair0 = 3, not handed to the kernel


def test_many_interleaves_what_it_says():
    c = sc.case("many", "five_abutting")
    reads, bounds = sc.reads_of(c), sc.bounds(c)
    assert all(b1[0] < b0[1] for b0, b1 in zip(bounds, bounds[1:])) and c.rate == 1.0          # the flanks overlap
    assert all(i0[1] == i1[0] for i0, i1 in zip(c.intervals, c.intervals[1:]))                  # the intervals abut
    pairs = [len(p) for _a, _b, p in c.intervals]
    n = c.expect["n"]
    assert 0 < n[0] < c.cap and pairs[0] <= c.cap                         # fewer reads than the cap
    assert n[1] > c.cap and "D" in c.intervals[1][2].strip("D")           # sampled, dead pairs between reads
    assert n[2] > c.cap and pairs[2] == n[2]                              # sampled
    assert n[3] == 0 and pairs[3] > c.cap                                 # all dead, and handed to the kernel
    assert n[4] == c.cap == pairs[4]                                      # n == cap
    kept = [{r["name"] for r in sc.kept_reads(c, r)} for r in (1, 2)]
    both = [{reads[i]["name"] for i, live in sc.pairs_of(reads, *bounds[r]) if live} for r in (1, 2)]
    shared = both[0] & both[1]
    assert len(shared) >= sc.MANY_SPAN
    assert (shared & kept[0]) - kept[1] and (shared & kept[1]) - kept[0] and shared & kept[0] & kept[1]
