"""pa_stitcher_variants through DeviceStitcher.variants(): the device's records against the numpy twin (Variants.records_numpy)
as bytes, and both against the per-hunk restatement of the rule (tests/polish_vcf_cases.py) -- contigs of a few hundred letters
at most, chosen where the kernels can go wrong: shifts on both sides of a 64-lane step, periods above one, the bound, the contig's
start, trimming.  The rule itself is held to its properties in tests/test_polish_vcf_cpu.py."""
import ctypes

import numpy as np
import pytest

import polish_vcf_cases as vcases
import test_gpu_polish_edits as ecases
from pepper_amd import _lib
from pepper_amd.polish import Edits, Variants
from pepper_amd.polish.DeviceStitch import DeviceStitcher

pytestmark = pytest.mark.gpu

KEY = ecases.KEY
A, C, G, T = 1, 2, 3, 4


def _feed(st, contig, keys, phred):
    table = {(int(p), int(i)): (int(label), int(q)) for p, i, label, q in zip(*keys, phred)}
    ecases._add_rows(st, contig, table, chunk=53, phred=True)


def _check(st, contig, draft, keys, phred=None, qualities=True):
    """One contig held by `st`: its filled finish, then the variants against the twin and the restatement.
    -> ([(POS, REF, ALT)], counts, records)."""
    if phred is None:
        phred = np.full(keys[0].size, 40, np.int64)
    if qualities:
        sequence, _ = st.finish(contig, 1, [KEY], qualities=True, fill=draft)
    else:
        sequence = st.finish(contig, 1, [KEY], fill=draft)
    edit_records, pieces, consensus = vcases.filled(draft, keys, phred if qualities else np.zeros(keys[0].size, np.int64))
    assert sequence == consensus
    before = st.stats()["table_bytes"]
    records = st.variants(draft)
    want, want_counts = Variants.records_numpy(edit_records, draft, consensus, qualities)
    assert records.dtype == Variants.VARIANT_DTYPE and records.tobytes() == want.tobytes()
    assert st.last_variant_counts == want_counts
    # the edit records it made (16 bytes each), 4 bytes per edit record, 69 per hunk, 32 per record
    grown = before + 20 * len(edit_records) + 69 * sum(want_counts[:3]) + 32 * want_counts[0]
    assert st.stats()["table_bytes"] == grown
    again = st.variants(draft)                                        # the same bytes again, counted once
    assert again.tobytes() == records.tobytes() and st.stats()["table_bytes"] == grown
    restated, restated_counts = vcases.restated(edit_records, pieces, draft, consensus, qualities)
    calls = Variants.alleles(records, draft, consensus)
    assert calls == [r[:3] for r in restated] and want_counts == restated_counts
    assert [int(q) for q in records["phred"]] == [r[3] if qualities else 0 for r in restated]
    if want_counts[2] == 0:
        assert Variants.replay(draft, calls) == consensus.upper()
    return calls, want_counts, records


def _one(draft, changes, qualities=True, **kw):
    keys = vcases.keys_of(draft, changes, **kw)
    phred = 10 + np.arange(keys[0].size) % 50
    with DeviceStitcher(0) as st:
        if qualities:
            _feed(st, "c", keys, phred)
        else:
            table = {(int(p), int(i)): (int(label), 0) for p, i, label in zip(*keys)}
            ecases._add_rows(st, "c", table, chunk=53, phred=False)
        return _check(st, "c", draft, keys, phred, qualities)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 200])
def test_indels_at_the_right_end_of_a_homopolymer(n):
    draft = "C" + "A" * n + "GT"
    calls, counts, records = _one(draft, {(n, 1): A})
    assert calls == [(1, "C", "CA")] and counts == [1, 0, 0, 1, n] and records["lead"].tolist() == [2]
    calls, counts, _ = _one(draft, {(n, 0): 0})
    assert calls == [(1, "CA", "C")] and counts == [1, 0, 0, int(n > 1), n - 1]
    # the run begins the contig: the anchor is the run's first letter, one place less
    calls, counts, _ = _one(draft[1:], {(n - 1, 1): A})
    assert calls == [(1, "A", "AA")] and counts[4] == n - 1


def test_deletions_in_a_repeat_of_period_two():
    draft = "GT" + "AC" * 40 + "TG"
    assert _one(draft, {(80, 0): 0, (81, 0): 0})[0] == [(2, "TAC", "T")]
    calls, counts, _ = _one(draft, {(p, 0): 0 for p in range(78, 82)})
    assert calls == [(2, "TACAC", "T")] and counts == [1, 0, 0, 1, 76]
    calls, counts, _ = _one(draft, {(p, 0): 0 for p in range(77, 81)})      # CACA, off the period's phase
    assert calls == [(2, "TACAC", "T")] and counts[4] == 75


def test_insertions_longer_and_shorter_than_their_shift():
    draft = "G" + "AC" * 3 + "TT"
    changes = {(6, i + 1): (A, C)[i % 2] for i in range(8)}          # ACACACAC behind ACACAC: 6 places, 8 letters
    calls, counts, records = _one(draft, changes)
    assert calls == [(1, "G", "GACACACAC")] and counts[4] == 6 and records["lead"].tolist() == [7]
    draft = "G" + "AC" * 40 + "TT"
    calls, counts, records = _one(draft, {(80, 1): A, (80, 2): C})     # AC behind 40 of them: 80 places, 2 letters
    assert calls == [(1, "G", "GAC")] and counts[4] == 80 and records["lead"].tolist() == [3]


@pytest.mark.parametrize("distance", [1, 2, 3])
def test_a_shift_stops_at_the_hunk_in_front(distance):
    draft = "T" + "A" * 20 + "G"
    calls, counts, _ = _one(draft, {(5, 0): C, (6 + distance, 0): 0})
    assert calls == [(6, "A", "C"), (7, "AA", "A")] and counts[4] == distance - 1
    calls, counts, _ = _one(draft, {(5, 0): 0, (6 + distance, 1): A})      # a deletion in front: it moved itself, its b0 did not
    assert calls == [(1, "TA", "T"), (7, "A", "AA")] and counts[4] == 4 + distance


def test_a_shift_through_a_filled_run():
    draft = "G" + "AA" + "aaaa" + "AAA" + "T"
    calls, counts, _ = _one(draft, {(9, 0): 0}, holes=(3, 4, 5, 6))
    assert calls == [(1, "GA", "G")] and counts[4] == 8
    draft = "G" + "AA" + "aNa" + "AAA" + "T"                          # the N stops it
    calls, counts, _ = _one(draft, {(8, 0): 0}, holes=(3, 4, 5))
    assert calls == [(5, "NA", "N")] and counts[4] == 3
    draft = "cg" + "tttt" + "ACGT"                                    # out of the piece, to a lower-case anchor in front of it
    calls, counts, _ = _one(draft, {(6, 0): 0, (6, 1): T, (6, 2): A}, first=6)
    assert calls == [(2, "G", "GT")] and counts[4] == 4


def test_hunks_that_trim():
    draft = "GATTACAGGC"
    # sub + ins + del that spell a SNV: GA[TT]AC -> GA[CT]AC
    calls, counts, _ = _one(draft, {(2, 0): C, (2, 1): T, (3, 0): 0})
    assert calls == [(3, "T", "C")] and counts == [1, 0, 0, 0, 0]
    # a gap at (3, 0) under T, T: the deleted T comes back and one more: an inserted T, which moves to the A in front of the run
    calls, counts, _ = _one(draft, {(3, 0): 0, (3, 1): T, (3, 2): T})
    assert calls == [(2, "A", "AT")] and counts == [1, 0, 0, 1, 1]
    # a gap at (5, 0) under the draft's own letter: nothing changed
    calls, counts, _ = _one(draft, {(5, 0): 0, (5, 1): C})
    assert calls == [] and counts == [0, 1, 0, 0, 0]
    # the no-op does not move the bound of the hunk behind it: its untrimmed end stands
    calls, counts, _ = _one("GAAAAAAT", {(2, 0): 0, (2, 1): A, (6, 0): 0})
    assert calls == [(4, "AA", "A")] and counts == [1, 1, 0, 1, 2]


def test_the_contigs_start():
    draft = "GAAAACGT"
    calls, counts, records = _one(draft, {(0, 0): 0, (4, 0): 0})       # F = 1: the deleted G leans on the A behind it
    assert calls == [(1, "GA", "A"), (3, "AA", "A")] and counts == [2, 0, 0, 1, 1] and records["tail"].tolist() == [1, 0]
    calls, counts, records = _one(draft, {(0, 0): 0, (2, 0): 0, (6, 1): G})      # F = 2: two of them, one letter apart
    assert calls == [(1, "GA", "A"), (3, "AA", "A"), (6, "C", "CG")] and records["tail"].tolist() == [1, 1, 0]
    assert counts == [3, 0, 0, 1, 1]
    calls, counts, records = _one(draft, {(0, 0): 0, (0, 1): T, (0, 2): G})      # trims to an insertion in front of the first letter
    assert calls == [(1, "G", "TG")] and records["tail"].tolist() == [1] and records["kind"].tolist() == [Variants.KIND_INS]
    calls, counts, _ = _one("ACG", {(0, 0): 0, (1, 0): 0, (2, 0): 0})            # nothing is left to lean on
    assert calls == [] and counts == [0, 0, 1, 0, 0]
    calls, counts, _ = _one("ACG", {(0, 0): 0, (2, 0): 0})                      # ... nor here: a chain from end to end
    assert calls == [(1, "AC", "C")] and counts == [1, 0, 1, 0, 0]


def test_the_contigs_end_no_edits_and_no_qualities():
    draft = "ACGTTGCATT"
    assert _one(draft, {(9, 1): C})[0] == [(10, "T", "TC")]
    assert _one(draft, {(9, 1): T})[0] == [(8, "A", "AT")]
    calls, counts, records = _one(draft, {})
    assert calls == [] and counts == [0] * 5 and len(records) == 0
    calls, counts, records = _one(draft, {}, first=2, last=7, holes=(4,))       # GAP records alone
    assert calls == [] and counts == [0] * 5
    calls, counts, records = _one(draft, {(3, 0): 0, (6, 0): A}, qualities=False)
    assert calls == [(3, "GT", "G"), (7, "C", "A")] and records["phred"].tolist() == [0, 0]
    _, _, text = Variants.lines("c", records, draft, "ACGTGAATT", False)
    assert text[0] == b"c\t3\t.\tGT\tG\t.\tPASS\t.\tGT\t1\n"


def test_two_contigs_and_random_ones_through_one_handle():
    rng = np.random.default_rng(77)
    cases = [vcases.random_case(rng) for _ in range(200)]
    cases = [c for c in cases if c[1][0].size]
    with DeviceStitcher(0) as st:
        for k, (draft, keys, phred) in enumerate(cases):
            _feed(st, "c%d" % k, keys, phred)
        total = np.zeros(5, np.int64)
        for k, (draft, keys, phred) in enumerate(cases):
            total += _check(st, "c%d" % k, draft, keys, phred)[1]
        first = _check(st, "c0", *cases[0])                            # an earlier contig again, behind all the others
        assert first[1] == _check(st, "c0", *cases[0])[1]
    assert total[0] > 150 and total[3] > 10


def test_refusals():
    lib = _lib.load()
    draft = b"ACGTACGT"
    n, counts = ctypes.c_int64(), (ctypes.c_int64 * 5)()
    out = np.zeros(4, Variants.VARIANT_DTYPE)

    def refused(rc):
        with pytest.raises(_lib.PepperAmdError) as error:
            _lib.check(rc)
        assert error.value.code == _lib.PA_ERR_INVALID

    with DeviceStitcher(0) as st:
        run = lambda d, length: lib.pa_stitcher_variants(st.handle, d, length, ctypes.byref(n), counts)
        take = lambda capacity: lib.pa_stitcher_take_variants(st.handle, out.ctypes.data, capacity)
        refused(run(draft, 8))                                         # no finish yet
        refused(take(4))
        keys = vcases.keys_of(draft.decode(), {(3, 0): 0, (5, 0): A})
        _feed(st, "c", keys, np.full(keys[0].size, 30))
        _feed(st, "bad", (np.array([0]), np.array([0]), np.array([9])), [1])
        with pytest.raises(KeyError):
            st.finish("bad", 1, [KEY])
        refused(run(draft, 8))                                         # no sequence
        st.finish("c", 1, [KEY])
        refused(run(draft, 8))                                         # no fill since the finish
        refused(take(4))
        st.finish("c", 1, [KEY], fill=draft)
        refused(run(draft, 7))                                         # not the fill's length
        refused(run(None, 9))
        refused(take(4))                                               # no run yet
        st.edits(draft)                                                # (reads the fill's copy: it stays)
        k6 = (ctypes.c_int64 * 6)()
        _lib.check(lib.pa_stitcher_edits(st.handle, draft, 8, ctypes.byref(n), k6))      # a draft of its own: the copy is gone
        refused(run(None, 8))
        _lib.check(run(draft, 8))                                      # and the handle is as usable as before
        assert n.value == 2 and list(counts) == [2, 0, 0, 0, 0]
        refused(take(1))                                               # short capacity
        _lib.check(take(2))
        _lib.check(run(None, 8))                                       # the upload of the last run serves this one
        again = np.zeros(2, Variants.VARIANT_DTYPE)
        _lib.check(lib.pa_stitcher_take_variants(st.handle, again.ctypes.data, 2))
        assert again.tobytes() == out[:2].tobytes()
        assert Variants.alleles(again, draft, "ACGAAGT") == [(3, "GT", "G"), (6, "C", "A")]
        st.finish("c", 1, [KEY])
        refused(take(4))                                               # a later finish invalidates them
