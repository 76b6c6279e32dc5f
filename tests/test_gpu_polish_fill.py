"""The filled consensus of the device stitch (pa_stitcher_fill through DeviceStitcher.finish(fill=)) against the host form
(pepper_amd/polish/Stitch.filled_piece, Edits.records_numpy(filled=True)): sequence, qualities and records byte for byte; the
files of stitch_directory against perform_stitch's.  The host form itself is held to its invariants in
tests/test_polish_fill_cpu.py.  Rows are fed straight to a DeviceStitcher, in chunks of 37 to 61 rows."""
import ctypes

import numpy as np
import pytest

import polish_edits_cases as cases
import test_gpu_polish_edits as ecases
from pepper_amd import _lib
from pepper_amd.polish import Edits, Stitch
from pepper_amd.polish.DeviceStitch import DeviceStitcher, stitch_directory
from pepper_amd.polish.Stitch import create_consensus_sequence
from pepper_amd.polish.perform_stitch import perform_stitch

pytestmark = pytest.mark.gpu

KEY = ecases.KEY
_DECODE = np.frombuffer(b"\0ACGT", dtype=np.uint8)
SUFFIXES = ("_pepper_polished.fa", "_pepper_polished.fastq", "_pepper_polished.edits.tsv")


def _host(table, draft, phred=True):
    """The host form on one region's table: (sequence, quality or None, records, pieces)."""
    keys = sorted(table)
    positions, indices = np.array([k[0] for k in keys], np.int64), np.array([k[1] for k in keys], np.int64)
    labels, q = np.array([table[k][0] for k in keys], np.int64), np.array([table[k][1] for k in keys], np.int64)
    letters = _DECODE[labels]
    quality = (33 + np.minimum(q[letters != 0], 93)).astype(np.uint8) if phred else None
    text, quality = Stitch.filled_piece(np.frombuffer(draft.encode(), np.uint8), int(positions[0]), positions, letters, quality)
    records = Edits.records_numpy(positions, indices, labels, q if phred else None, draft, filled=True)
    sequence = text.tobytes().decode()
    return sequence, quality.tobytes().decode() if phred else None, records, [(int(positions[0]), int(positions[-1]), len(sequence))]


def _run(table, draft, phred=True, chunk=61, threads=1):
    """One stitcher fed the table: the filled finish, then its edits, against the host form; the unfilled finish of the same
    handle is the filled one with its runs cut out.  -> (sequence, records, fill counts)."""
    want_sequence, want_quality, want_records, want_pieces = _host(table, draft, phred)
    with DeviceStitcher(0) as st:
        ecases._add_rows(st, "c", table, chunk=chunk, phred=phred)
        unfilled = st.finish("c", 1, [KEY])
        before = st.stats()
        if phred:
            sequence, quality = st.finish("c", threads, [KEY], qualities=True, fill=draft)
            assert quality == want_quality
        else:
            sequence = st.finish("c", threads, [KEY], fill=draft)
        assert sequence == want_sequence and st.pieces() == want_pieces
        stats = st.stats()
        assert stats["table_bytes"] == before["table_bytes"] + 4 * stats["positions"] + len(sequence) * (2 if phred else 1)
        counts = st.last_fill_counts
        records = st.edits(draft)
        ecases._same(records, want_records)
        assert st.stats()["table_bytes"] == stats["table_bytes"] + 16 * len(records)
    assert Edits.apply_filled(draft, records, want_pieces) == sequence
    hunks = Edits.filled_hunks(records, want_pieces, len(draft), phred)
    runs = [h for h in hunks if h[4] == "filled"]
    assert counts == [len(runs), sum(h[1] - h[0] for h in runs)]
    cut, at = [], 0
    for h in runs:
        assert sequence[h[2]:h[3]] == draft[h[0]:h[1]]
        cut.append(sequence[at:h[2]])
        at = h[3]
    assert ''.join(cut) + sequence[at:] == unfilled
    return sequence, records, counts


def _marked_draft(rng, n):
    """A draft with lower-case letters and Ns all over."""
    draft = list(cases.random_draft(rng, n))
    for p in rng.integers(0, n, n // 5).tolist():
        draft[p] = draft[p].lower()
    for p in rng.integers(0, n, n // 40 + 1).tolist():
        draft[p] = "N"
    return ''.join(draft)


def _table(draft, a, b, phred=40):
    return {(p, 0): (cases.CODE.get(draft[p].upper(), 1), phred) for p in range(a, b)}


@pytest.mark.parametrize("phred", [True, False])
@pytest.mark.parametrize("case", ["leading", "trailing", "neither"])
def test_runs_at_the_ends(case, phred):
    rng = np.random.default_rng(5)
    draft = _marked_draft(rng, 200)
    a, b = {"leading": (30, 200), "trailing": (0, 150), "neither": (0, 200)}[case]
    table = _table(draft, a, b)
    table[(a, 0)] = (cases.other(draft[a]), 3)
    table[(b - 1, 1)] = (2, 99)
    sequence, records, counts = _run(table, draft, phred)
    assert counts == [0 if case == "neither" else 1, 200 - (b - a)] and len(sequence) == 201
    assert sequence[:a] == draft[:a] and (b == 200 or sequence[-50:] == draft[150:])


@pytest.mark.parametrize("phred", [True, False])
def test_interior_runs_of_one_and_of_hundreds(phred):
    rng = np.random.default_rng(6)
    draft = _marked_draft(rng, 1500)
    table = _table(draft, 3, 1490)
    del table[(100, 0)]
    for p in range(400, 900):
        del table[(p, 0)]
    for k, p in enumerate(range(10, 1490, 97)):
        if (p, 0) in table:
            table[(p, 0)] = (0, k) if k % 2 else (cases.other(draft[p]), k)
            table[(p, 2)] = (1 + k % 4, 200 + k)
    sequence, records, counts = _run(table, draft, phred, chunk=37)
    assert counts == [4, 3 + 1 + 500 + 10]
    gaps = records[records["kind"] == Edits.GAP_OPEN]
    assert gaps["position"].tolist() == [100, 400] and all(sequence[o] == draft[p] for p, o in zip([100, 400], gaps["offset"].tolist()))


def test_insert_slots_without_a_writer_beside_a_run():
    """Positions whose only keys are insert slots -- (p, 0) has no writer -- right in front of a run and right behind one: they
    have a slot, so they are not filled, and give a DEL."""
    rng = np.random.default_rng(7)
    draft = _marked_draft(rng, 300)
    table = _table(draft, 10, 290)
    for p in range(100, 120):
        del table[(p, 0)]
    table[(100, 1)] = (3, 50)                      # a slot in front of the run 101..118
    table[(119, 2)] = (4, 60)                      # and one behind it
    del table[(200, 0)]
    del table[(201, 0)]
    table[(200, 1)] = (0, 70)                      # a gap in an insert slot: a slot, no letter; the run is 201 alone
    for i in range(1, 301):                        # one position with 300 insert slots (some empty, some gaps) behind a run
        if i % 7:
            table[(202, i)] = (int(rng.integers(0, 5)), i % 256)
    sequence, records, counts = _run(table, draft)
    assert counts == [4, 10 + 18 + 1 + 10] and int(records["index"].max()) == 300
    by_key = {(int(r["position"]), int(r["kind"])) for r in records}
    assert {(100, 2), (100, 3), (101, 4), (118, 5), (119, 2), (119, 3), (200, 2), (201, 4), (201, 5)} <= by_key


@pytest.mark.parametrize("phred", [True, False])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_runs_at_the_scan_block(d, phred):
    """Runs that end, begin or lie one position in front of, at and behind a workgroup boundary of the scans.  Inserts in front
    make up for the positions a run takes away, so the slot behind every run sits at the same place among the slots."""
    B = DeviceStitcher.limits()["scan_block"]
    assert B == 1024
    rng = np.random.default_rng(40 + d)
    first, size = 7, 3 * B + 50
    draft = _marked_draft(rng, first + size + 3)
    table = _table(draft, first, first + size)
    at = lambda index: first + index
    for k in range(1, 4):
        table[(at(2), k)] = (k, 10 + k)                                # three inserts: the slot of index B + d is slot B + d
    for index in range(B + d - 3, B + d):                             # a run that ends at index B + d - 1
        del table[(at(index), 0)]
    for index in range(2 * B + d, 2 * B + d + 5):                     # a run that begins at index 2 B + d
        del table[(at(index), 0)]
    for k in range(1, 6):
        table[(at(2 * B + d + 5), k)] = (1 + k % 4, 20 + k)            # five more: index 3 B + d + 1 is slot 3 B + d + 1
    del table[(at(3 * B + d), 0)]                                     # one position, at index 3 B + d
    if (at(B - 1), 0) in table:                                       # edits at the boundaries, where a run does not take them
        table[(at(B - 1), 0)] = (cases.other(draft[at(B - 1)]), 1)
    if (at(2 * B), 0) in table:
        table[(at(2 * B), 0)] = (0, 2)
    sequence, records, counts = _run(table, draft, phred)
    assert counts == [5, first + 3 + 5 + 1 + 3]
    with DeviceStitcher(0) as st:
        ecases._add_rows(st, "c", table, phred=phred)
        st.finish("c", 1, [KEY], fill=draft)
        stats = st.stats()
    assert stats["positions"] == size >= 2 * B + 1 and stats["slots"] == size - 9 + 8


def test_threads_do_not_change_the_plan():
    draft = _marked_draft(np.random.default_rng(8), 500)
    table = _table(draft, 20, 480)
    del table[(250, 0)]
    assert _run(table, draft, threads=1)[0] == _run(table, draft, threads=7)[0]


# ---- several regions, from prediction files ----
def _host_files(pred, draft_fa, where, threads, **kw):
    kw = dict(dict(qualities=True, edits=draft_fa, fill=draft_fa), **kw)
    perform_stitch(str(pred), str(where), threads, **kw)
    return tuple(open(str(where) + suffix).read() for suffix in SUFFIXES)


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fill_planted")
    draft = list(cases.write_planted(tmp / "pred")["ctg"])
    for p in (0, 3, 120, 265, 270, 399):
        draft[p] = draft[p].lower()
    draft[5] = draft[266] = draft[360] = "N"
    drafts = {"b1": "acgtNNacgtTTGGaa" * 9, "ctg": ''.join(draft), "ctg2": "ttAAccNn"}
    draft_fa = cases.write_draft(tmp / "draft.fa", drafts)
    want = create_consensus_sequence("ctg", cases.contig_keys(tmp / "pred", "ctg"), 1, qualities=True, edits=draft_fa, fill=draft_fa)
    return tmp / "pred", draft_fa, drafts, want, tmp


@pytest.mark.parametrize("phred", [True, False])
def test_regions_shuffled_split_adds_and_device_tensors(planted, phred):
    pred, draft_fa, drafts, (want_sequence, want_quality, want_records, want_pieces), _ = planted
    if not phred:
        _, _, want_records, _ = create_consensus_sequence("ctg", cases.contig_keys(pred, "ctg"), 1, edits=draft_fa, fill=draft_fa)
        want_records = want_records.copy()
        want_records["phred"] = 0                  # (the files hold a phred; a contig fed without one has none)
    for shuffle, threads in ((None, 1), (8, 3), (9, 8)):
        with DeviceStitcher(0) as st:
            keys = ecases._feed(st, pred, "ctg", phred=phred, shuffle=shuffle, device=shuffle is not None)
            if phred:
                assert st.finish("ctg", threads, keys, qualities=True, fill=drafts["ctg"]) == (want_sequence, want_quality)
            else:
                assert st.finish("ctg", threads, keys, fill=drafts["ctg"].encode()) == want_sequence
            assert st.pieces() == want_pieces
            records = st.edits(drafts["ctg"])
            ecases._same(records, want_records)
            assert st.last_fill_counts == [4, 10 + 1 + 19 + 49]
    assert Edits.apply_filled(drafts["ctg"], records, want_pieces) == want_sequence


@pytest.mark.parametrize("unpolished", [False, True])
def test_stitch_directory_and_writers_write_the_host_files(planted, unpolished):
    pred, draft_fa, drafts, want, tmp = planted
    tag = "all" if unpolished else "only"
    host = _host_files(pred, draft_fa, tmp / ("host_" + tag) / "asm", 3, unpolished_contigs=unpolished)
    stats = {}
    out = stitch_directory(str(pred), str(tmp / ("dev_" + tag) / "asm"), 3, stats=stats, qualities=True, edits=draft_fa, fill=draft_fa,
                           unpolished_contigs=unpolished)
    assert tuple(open(out[:-len(SUFFIXES[0])] + suffix).read() for suffix in SUFFIXES) == host
    assert list(cases.fasta_sequences(host[0])) == (["b1", "ctg", "ctg2"] if unpolished else ["ctg"])
    assert stats["fill"]["runs"] == 4 and stats["fill"]["letters"] == 79 and stats["fill"]["seconds"] > 0
    with DeviceStitcher(0) as st:
        ecases._feed(st, pred, "ctg", shuffle=3)
        st.write_fastq(str(tmp / ("writer_" + tag) / "asm"), 2, edits=draft_fa, fill=draft_fa, unpolished_contigs=unpolished)
        assert tuple(open(str(tmp / ("writer_" + tag) / "asm") + suffix).read() for suffix in SUFFIXES) == host
        st.write_fasta(str(tmp / ("fasta_" + tag) / "asm"), 2, fill=draft_fa, unpolished_contigs=unpolished)
        assert open(str(tmp / ("fasta_" + tag) / "asm") + SUFFIXES[0]).read() == host[0]
        # and with fill off the handle writes what it wrote before
        st.write_fastq(str(tmp / ("off_" + tag) / "asm"), 3, edits=draft_fa)
        assert tuple(open(str(tmp / ("off_" + tag) / "asm") + suffix).read() for suffix in SUFFIXES) == \
            _host_files(pred, draft_fa, tmp / ("hostoff_" + tag) / "asm", 3, fill=None)


# ---- the C entry point: the order of fill and edits, a second finish, the refusals ----
class _Calls(object):
    def __init__(self, st):
        self.lib, self.st = _lib.load(), st
        self.n, self.counts, self.total, self.fill_counts = ctypes.c_int64(), (ctypes.c_int64 * 6)(), ctypes.c_int64(), (ctypes.c_int64 * 2)()

    def fill(self, draft):
        return self.lib.pa_stitcher_fill(self.st.handle, draft, len(draft), ctypes.byref(self.total), self.fill_counts)

    def edits(self, draft, length=None):
        return self.lib.pa_stitcher_edits(self.st.handle, draft, len(draft) if length is None else length, ctypes.byref(self.n), self.counts)

    def take(self, n, qualities=False):
        buf = ctypes.create_string_buffer(max(1, n))
        take = self.lib.pa_stitcher_take_qualities if qualities else self.lib.pa_stitcher_take
        assert take(self.st.handle, buf, n) == _lib.PA_OK
        return buf.raw[:n].decode()

    def take_edits(self):
        records = np.zeros(self.n.value, Edits.EDIT_DTYPE)
        assert self.lib.pa_stitcher_take_edits(self.st.handle, records.ctypes.data, self.n.value) == _lib.PA_OK
        return records

    def error(self):
        return self.lib.pa_last_error()


def test_fill_and_edits_in_either_order_and_a_second_finish(planted):
    pred, draft_fa, drafts, (want_sequence, want_quality, want_records, want_pieces), _ = planted
    draft = drafts["ctg"].encode()
    unfilled_sequence, unfilled_quality, unfilled_records, _ = create_consensus_sequence("ctg", cases.contig_keys(pred, "ctg"), 1,
                                                                                         qualities=True, edits=draft_fa)
    with DeviceStitcher(0) as st:
        c = _Calls(st)
        keys = ecases._feed(st, pred, "ctg")
        # edits, then fill: the records of the unfilled consensus first; the fill drops them, the next edits gives the filled ones
        assert st.finish("ctg", 1, keys, qualities=True) == (unfilled_sequence, unfilled_quality)
        bare = st.stats()["table_bytes"]
        assert c.edits(draft) == _lib.PA_OK
        ecases._same(c.take_edits(), unfilled_records)
        assert c.fill(draft) == _lib.PA_OK and c.total.value == len(want_sequence) and list(c.fill_counts) == [4, 79]
        assert c.take(c.total.value) == want_sequence and c.take(c.total.value, qualities=True) == want_quality
        assert c.lib.pa_stitcher_take_edits(st.handle, None, 0) == _lib.PA_ERR_INVALID and b"has not run" in c.error()
        filled_bytes = 4 * st.stats()["positions"] + 2 * len(want_sequence)
        assert st.stats()["table_bytes"] == bare + filled_bytes
        assert c.edits(draft) == _lib.PA_OK                          # (a draft of the caller's: uploaded again, the same records)
        ecases._same(c.take_edits(), want_records)
        # fill, then edits with the draft the fill left on the device; asked twice: counted once
        assert c.fill(draft) == _lib.PA_OK and c.edits(None, len(draft)) == _lib.PA_OK
        ecases._same(c.take_edits(), want_records)
        assert st.stats()["table_bytes"] == bare + filled_bytes + 16 * len(want_records)
        assert c.take(c.total.value) == want_sequence
        # a second finish drops the filled state
        assert st.finish("ctg", 1, keys, qualities=True) == (unfilled_sequence, unfilled_quality)
        assert st.stats()["table_bytes"] == bare
        assert c.edits(None, len(draft)) == _lib.PA_ERR_INVALID and b"null draft" in c.error()
        ecases._same(st.edits(draft), unfilled_records)
        assert st.finish("ctg", 4, keys, qualities=True, fill=draft) == (want_sequence, want_quality)
        ecases._same(st.edits(draft), want_records)


def test_refusals_leave_the_handle_usable(planted):
    pred, draft_fa, drafts, (want_sequence, want_quality, want_records, want_pieces), _ = planted
    draft = drafts["ctg"].encode()

    def good(st, keys):
        assert st.finish("ctg", 2, keys, qualities=True, fill=draft) == (want_sequence, want_quality)
        ecases._same(st.edits(draft), want_records)

    with DeviceStitcher(0) as st:
        c = _Calls(st)
        assert c.fill(draft) == _lib.PA_ERR_INVALID and b"no contig has been finished" in c.error()
        keys = ecases._feed(st, pred, "ctg")
        good(st, keys)
        # a finish with more than one piece
        unfilled = st.finish("ctg", 3, keys)
        assert len(st.pieces()) == 2
        assert c.fill(draft) == _lib.PA_ERR_INVALID and b"2 pieces" in c.error()
        assert c.take(len(unfilled)) == unfilled                     # the handle still speaks of that finish
        good(st, keys)
        # a draft that does not reach the piece's last position, 350
        st.finish("ctg", 1, keys)
        assert c.fill(draft[:350]) == _lib.PA_ERR_INVALID and b"350" in c.error()
        assert c.fill(draft[:351]) == _lib.PA_OK and c.take(c.total.value) == want_sequence[:-49]
        length = c.total.value
        assert c.fill(draft[:350]) == _lib.PA_ERR_INVALID and c.total.value == 0      # refused after a fill: the filled consensus stays
        assert c.take(length) == want_sequence[:-49]
        buf = ctypes.create_string_buffer(8)
        assert c.lib.pa_stitcher_take(st.handle, buf, 8) == _lib.PA_ERR_INVALID and b"room for" in c.error()
        good(st, keys)
        # a finish that gives no sequence: a label that is no base
        st.add("bad", [KEY], [0], np.arange(4).reshape(1, 4), np.zeros((1, 4), np.int64), np.array([[1, 7, 2, 3]], np.uint8),
               np.zeros((1, 4), np.uint8))
        with pytest.raises(KeyError):
            st.finish("bad", 1, [KEY], fill=b"ACGTACGT")
        assert c.fill(b"ACGTACGT") == _lib.PA_ERR_INVALID and b"no sequence" in c.error()
        good(st, keys)
        # a contig the handle holds nothing of: the draft as it is
        assert st.finish("nothing", 1, [], qualities=True, fill="acgtN") == ("acgtN", "!!!!!")
        assert st.pieces() == [] and len(st.edits("acgtN")) == 0 and st.last_fill_counts == [1, 5]
        good(st, keys)
