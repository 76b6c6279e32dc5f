"""min_quality polish on the device (pa_stitcher_gate / pa_stitcher_take_withheld through DeviceStitcher.finish(min_quality=) and
withheld()) against the host twin (pepper_amd/polish/Stitch.py gate_numpy, held to a hand-written case in
tests/test_polish_gate_cpu.py): sequence, qualities, pieces, applied edits and withheld records byte for byte; the invariants that
need no twin; the scan boundary; a second finish; every refusal; and the four files of the writers against perform_stitch's."""
import ctypes

import numpy as np
import pytest

import polish_edits_cases as cases
import test_gpu_polish_edits as ecases
import test_polish_gate_cpu as gcases
from pepper_amd import _lib
from pepper_amd.polish import Edits, Stitch
from pepper_amd.polish.DeviceStitch import DeviceStitcher, stitch_directory
from pepper_amd.polish.Stitch import create_consensus_sequence
from pepper_amd.polish.perform_stitch import perform_stitch

pytestmark = pytest.mark.gpu

KEY = ecases.KEY
SUFFIXES = gcases.SUFFIXES


def _host(table, draft, q, fill):
    """The host form on one region's table: (sequence, quality, applied records, pieces, withheld records)."""
    positions, indices, labels, phred, withheld = gcases._gate(table, draft, q, filled=fill)
    letters = Stitch._DECODE[labels]
    quality = (33 + np.minimum(phred[letters != 0], 93)).astype(np.uint8)
    text = letters[letters != 0]
    if fill:
        text, quality = Stitch.filled_piece(np.frombuffer(draft.encode(), np.uint8), int(positions[0]), positions, letters, quality)
    records = Edits.records_numpy(positions, indices, labels, phred, draft, filled=fill)
    sequence = text.tobytes().decode()
    return sequence, quality.tobytes().decode(), records, [(int(positions[0]), int(positions[-1]), len(sequence))], withheld


def _run(table, draft, q, fill, chunk=61):
    """One stitcher fed the table: the gated finish, the withheld records and the edits behind it against the host form.
    -> (sequence, applied records, withheld records, stats after the gate)"""
    want_sequence, want_quality, want_records, want_pieces, want_withheld = _host(table, draft, q, fill)
    with DeviceStitcher(0) as st:
        ecases._add_rows(st, "c", table, chunk=chunk)
        sequence, quality = st.finish("c", 1, [KEY], qualities=True, fill=draft if fill else None, min_quality=q, draft=draft)
        assert sequence == want_sequence and quality == want_quality and st.pieces() == want_pieces
        withheld = st.withheld()
        ecases._same(withheld, want_withheld)
        assert st.last_gate_counts == [len(want_withheld)] + Edits.kind_counts(want_withheld)
        stats = st.stats()
        records = st.edits(draft)                                    # gate -> (fill ->) edits, the draft the gate left on the device
        ecases._same(records, want_records)
        ecases._same(st.withheld(), want_withheld)
    replay = Edits.apply_filled if fill else Edits.apply
    assert replay(draft, records, want_pieces) == sequence
    return sequence, records, withheld, stats


# ---- 1. the device against the host twin ----
@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("q", [1, 20, 255])
def test_one_piece_from_a_table(q, fill):
    """Every kind at every phred around the gate, lower-case letters and Ns in the draft, an empty (p, 0) beside insert slots, a
    position with 300 insert slots, an uncovered run."""
    rng = np.random.default_rng(q)
    draft = gcases._marked_draft(rng, 900)
    table = gcases._big_table(rng, draft, 20, 880)
    sequence, records, withheld, stats = _run(table, draft, q, fill, chunk=37 if fill else 61)
    assert stats["slots"] > 1100 and (len(withheld) > 50 or q == 1) and (int(withheld["index"].max(initial=0)) > 100 or q == 1)


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gate_planted")
    draft = list(cases.write_planted(tmp / "pred")["ctg"])
    for p in (0, 3, 20, 120, 265, 270, 300, 399):
        draft[p] = draft[p].lower()
    draft[5] = draft[266] = draft[360] = "N"
    drafts = {"b1": "acgtNNacgtTTGGaa" * 9, "ctg": ''.join(draft), "ctg2": "ttAAccNn"}
    return tmp / "pred", cases.write_draft(tmp / "draft.fa", drafts), drafts, tmp


@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("q", [1, 20, 255])
def test_pieces_from_prediction_files(planted, q, threads, fill):
    """Four regions: one piece with threads = 1, two overlapping ones with threads = 3 (one whatever the threads with fill); the
    adds shuffled, every other one with device tensors."""
    pred, draft_fa, drafts, _ = planted
    draft = drafts["ctg"]
    kw = dict(fill=draft_fa) if fill else {}
    want_sequence, want_quality, want_records, want_pieces, want_withheld = create_consensus_sequence(
        "ctg", cases.contig_keys(pred, "ctg"), threads, qualities=True, edits=draft_fa, min_quality=q, draft=draft_fa, **kw)
    assert len(want_pieces) == (1 if fill or threads == 1 else 2) and len(want_withheld) >= 2
    with DeviceStitcher(0) as st:
        keys = ecases._feed(st, pred, "ctg", shuffle=q + threads, device=True)
        got = st.finish("ctg", threads, keys, qualities=True, fill=draft if fill else None, min_quality=q, draft=draft)
        assert got == (want_sequence, want_quality) and st.pieces() == want_pieces
        ecases._same(st.withheld(), want_withheld)
        ecases._same(st.edits(draft), want_records)
        assert st.last_edit_counts[1:4] == Edits.kind_counts(want_records)
        # without qualities asked for, the same sequence
        assert st.finish("ctg", threads, keys, fill=draft if fill else None, min_quality=q, draft=draft) == want_sequence
        ecases._same(st.withheld(), want_withheld)


# ---- 2. invariants that need no twin ----
@pytest.mark.parametrize("fill", [False, True])
def test_a_gate_below_every_phred_changes_nothing(fill):
    rng = np.random.default_rng(77)
    draft = gcases._marked_draft(rng, 700)
    table = {key: (label, 5 + phred % 251) for key, (label, phred) in gcases._big_table(rng, draft, 10, 690).items()}
    mid = (10 + 690) // 2
    table[(mid + 11, 0)] = (0, 5)                                     # (no slot without a writer at index 0: those have phred 0)
    with DeviceStitcher(0) as st:
        ecases._add_rows(st, "c", table)
        ungated = st.finish("c", 1, [KEY], qualities=True, fill=draft if fill else None)
        records = st.edits(draft).tobytes()
        bare = st.stats()
        assert st.finish("c", 1, [KEY], qualities=True, fill=draft if fill else None, min_quality=5, draft=draft) == ungated
        assert st.last_gate_counts == [0, 0, 0, 0] and len(st.withheld()) == 0
        assert st.edits(draft).tobytes() == records and st.stats() == bare


def test_the_highest_gate_with_fill_reproduces_the_draft():
    """Q = 255 over phreds <= 254 withholds every edit, and with fill every position gives its draft letter: an upper-case ACGT
    draft comes back as it is."""
    rng = np.random.default_rng(78)
    draft = cases.random_draft(rng, 800)
    table = {key: (label, phred % 255) for key, (label, phred) in gcases._big_table(rng, draft, 15, 790).items()}
    with DeviceStitcher(0) as st:
        ecases._add_rows(st, "c", table)
        assert st.finish("c", 1, [KEY], fill=draft) != draft
        sequence, quality = st.finish("c", 1, [KEY], qualities=True, fill=draft, min_quality=255, draft=draft)
        assert sequence == draft and len(quality) == len(draft)
        records = st.edits(draft)
        assert not (records["kind"] < Edits.GAP_OPEN).any()
        withheld = st.withheld()
        assert st.last_gate_counts[0] == len(withheld) > 100
        for r in withheld[withheld["kind"] != Edits.INS]:            # a kept letter stands where the draft has it
            assert int(r["offset"]) == int(r["position"])


# ---- 3. the scan boundary ----
@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_withheld_edits_at_the_scan_block(d, fill):
    """A withheld DEL (a letter appears), a withheld INS (a letter disappears) and a withheld SUB in the slots B + d - 1, B + d,
    B + d + 1 and 2 B + d - 1, 2 B + d, 2 B + d + 1: over d they lie in front of, on and behind both workgroup boundaries of the
    scans, and every place behind them shifts."""
    B = DeviceStitcher.limits()["scan_block"]
    assert B == 1024
    rng = np.random.default_rng(50 + d)
    first, size = 7, 3 * B + 50
    draft = gcases._marked_draft(rng, first + size + 3)
    draft = ''.join("ACGT"[k % 4] if first + B - 4 <= k <= first + 2 * B + 4 and c not in "ACGT" else c for k, c in enumerate(draft))
    table = {(p, 0): (cases.CODE.get(draft[p].upper(), 1), 40) for p in range(first, first + size)}
    # (the draft has bases around both boundaries, so the gate has a letter to keep there)
    for at in (first + B + d - 1, first + 2 * B + d - 2):            # (the first insert slot moves every later slot up by one)
        table[(at, 0)] = (0, 3)
        table[(at, 1)] = (1 + at % 4, 4)
        table[(at + 1, 0)] = (cases.other(draft[at + 1]), 5)
    del table[(first + 40, 0)]                                       # one uncovered position in the first block, and an applied
    table[(first + 2, 1)] = (2, 50)                                  # insert in front of it: the slot of index k > 40 is slot k
    sequence, records, withheld, stats = _run(table, draft, 20, fill)
    assert stats["slots"] == size + 2 and stats["positions"] == size
    assert [(int(r["position"]) - first, int(r["index"]), int(r["kind"])) for r in withheld] == [
        (B + d - 1, 0, 2), (B + d - 1, 1, 3), (B + d, 0, 1), (2 * B + d - 2, 0, 2), (2 * B + d - 2, 1, 3), (2 * B + d - 1, 0, 1)]
    # letters in front of index k > 40: one per position, the applied insert for the uncovered position; with fill the draft's
    # letters in front of the piece and the filled position as well
    lead = first + 1 if fill else 0
    a, j = B + d - 1, 2 * B + d - 2
    assert [int(r["offset"]) - lead for r in withheld] == [a, a + 1, a + 1, j, j + 1, j + 1]


# ---- 4. a second finish ----
def test_a_second_finish_is_ungated_again(planted):
    pred, draft_fa, drafts, _ = planted
    draft = drafts["ctg"]
    keys_of = cases.contig_keys(pred, "ctg")
    ungated = create_consensus_sequence("ctg", keys_of, 3, qualities=True, edits=draft_fa)
    gated = create_consensus_sequence("ctg", keys_of, 3, qualities=True, edits=draft_fa, min_quality=20, draft=draft_fa)
    assert gated[0] != ungated[0]
    with DeviceStitcher(0) as st:
        keys = ecases._feed(st, pred, "ctg")
        for _ in range(2):
            assert st.finish("ctg", 3, keys, qualities=True) == ungated[:2]
            bare = st.stats()
            ecases._same(st.edits(draft), ungated[2])
            assert st.finish("ctg", 3, keys, qualities=True) == ungated[:2] and st.stats() == bare
            assert st.finish("ctg", 3, keys, qualities=True, min_quality=20, draft=draft) == gated[:2]
            stats = st.stats()
            # what the gate documents: 16 bytes per withheld record, and the quality buffer follows the sequence's length
            assert stats["table_bytes"] == bare["table_bytes"] + 16 * len(gated[4]) + len(gated[0]) - len(ungated[0])
            assert {k: v for k, v in stats.items() if k != "table_bytes"} == {k: v for k, v in bare.items() if k != "table_bytes"}
            ecases._same(st.withheld(), gated[4])
            ecases._same(st.edits(draft), gated[2])
            assert st.stats()["table_bytes"] == stats["table_bytes"] + 16 * len(gated[2])


# ---- 5. every refusal ----
class _Calls(object):
    def __init__(self, st, n_pieces=4):
        self.lib, self.st = _lib.load(), st
        self.total, self.counts, self.length = ctypes.c_int64(), (ctypes.c_int64 * 4)(), (ctypes.c_int64 * n_pieces)()
        self.filled, self.fill_counts = ctypes.c_int64(), (ctypes.c_int64 * 2)()

    def gate(self, draft, q, length=None):
        return self.lib.pa_stitcher_gate(self.st.handle, draft, len(draft) if length is None else length, q, self.length,
                                         ctypes.byref(self.total), self.counts)

    def fill(self, draft, length=None):
        return self.lib.pa_stitcher_fill(self.st.handle, draft, len(draft) if length is None else length, ctypes.byref(self.filled),
                                         self.fill_counts)

    def take_withheld(self, n):
        records = np.zeros(max(n, 0) + 1, Edits.EDIT_DTYPE)
        return self.lib.pa_stitcher_take_withheld(self.st.handle, records.ctypes.data, n), records[:max(n, 0)]

    def take(self, n):
        buf = ctypes.create_string_buffer(max(1, n))
        assert self.lib.pa_stitcher_take(self.st.handle, buf, n) == _lib.PA_OK
        return buf.raw[:n].decode()

    def error(self):
        return self.lib.pa_last_error()


def test_refusals_leave_the_handle_usable(planted):
    pred, draft_fa, drafts, _ = planted
    text = drafts["ctg"]
    draft = text.encode()
    keys_of = cases.contig_keys(pred, "ctg")
    ungated = create_consensus_sequence("ctg", keys_of, 3)
    want = create_consensus_sequence("ctg", keys_of, 3, qualities=True, edits=draft_fa, min_quality=20, draft=draft_fa)
    want_filled = create_consensus_sequence("ctg", keys_of, 3, qualities=True, fill=draft_fa, min_quality=20, draft=draft_fa)
    INVALID = _lib.PA_ERR_INVALID

    def good(st, keys):
        assert st.finish("ctg", 3, keys, qualities=True, min_quality=20, draft=text) == want[:2]
        ecases._same(st.withheld(), want[4])
        ecases._same(st.edits(text), want[2])

    with DeviceStitcher(0) as st:
        c = _Calls(st)
        assert c.gate(draft, 20) == INVALID and b"no contig has been finished" in c.error()
        assert c.take_withheld(8)[0] == INVALID and b"has not run" in c.error()
        keys = ecases._feed(st, pred, "ctg")
        good(st, keys)
        # after a finish: no gate yet, the range of min_phred, the draft's length (piece_last = 350)
        assert st.finish("ctg", 3, keys) == ungated
        assert c.take_withheld(8)[0] == INVALID and b"has not run" in c.error()
        for q in (0, -1, 256):
            assert c.gate(draft, q) == INVALID and b"outside 1..255" in c.error()
        assert c.gate(draft[:350], 20) == INVALID and b"350" in c.error()
        assert c.take(len(ungated)) == ungated                       # nothing changed
        assert c.gate(draft[:351], 20) == _lib.PA_OK and c.total.value == len(want[0]) and list(c.counts) == [7, 3, 2, 2]
        assert [int(v) for v in c.length][:2] == [p[2] for p in want[3]] and c.take(c.total.value) == want[0]
        # short capacity, then enough
        assert c.take_withheld(6)[0] == INVALID and b"room for" in c.error()
        rc, records = c.take_withheld(7)
        assert rc == _lib.PA_OK
        ecases._same(records, want[4])
        # a second gate, and a gate behind a fill
        assert c.gate(draft, 30) == INVALID and b"a gate already ran" in c.error()
        assert c.take(c.total.value) == want[0]
        good(st, keys)
        assert st.finish("ctg", 1, keys)
        assert c.fill(draft) == _lib.PA_OK
        assert c.gate(draft, 20) == INVALID and b"a fill already ran" in c.error()
        assert c.fill(None, len(draft)) == INVALID and b"null draft" in c.error()          # (no gate left a draft there)
        # gate, then a fill that reads the gate's draft
        assert st.finish("ctg", 1, keys)
        assert c.gate(draft, 20) == _lib.PA_OK and c.fill(None, len(draft)) == _lib.PA_OK and c.take(c.filled.value) == want_filled[0]
        ecases._same(c.take_withheld(7)[1], want_filled[2])
        good(st, keys)
        # a finish that gives no sequence: a label that is no base
        st.add("bad", [KEY], [0], np.arange(4).reshape(1, 4), np.zeros((1, 4), np.int64), np.array([[1, 7, 2, 3]], np.uint8),
               np.zeros((1, 4), np.uint8))
        with pytest.raises(KeyError):
            st.finish("bad", 1, [KEY], min_quality=20, draft="ACGTACGT")
        assert c.gate(b"ACGTACGT", 20) == INVALID and b"no sequence" in c.error()
        assert c.take_withheld(8)[0] == INVALID
        good(st, keys)
        # a contig with a chunk that came without qualities
        st.add("plain", [KEY], [0], np.arange(4).reshape(1, 4), np.zeros((1, 4), np.int64), np.array([[1, 2, 2, 3]], np.uint8),
               np.full((1, 4), 9, np.uint8))
        st.add("plain", [KEY], [1], np.arange(4, 8).reshape(1, 4), np.zeros((1, 4), np.int64), np.array([[1, 2, 2, 3]], np.uint8))
        assert st.finish("plain", 1, [KEY]) == "ACCGACCG"
        assert c.gate(b"ACGTACGT", 20) == INVALID and b"without qualities" in c.error()
        assert c.take(8) == "ACCGACCG"
        with pytest.raises(_lib.PepperAmdError):
            st.finish("plain", 1, [KEY], min_quality=20, draft="ACGTACGT")
        good(st, keys)
        # the Python surface: values outside the range, a gate without its draft
        for bad in (-1, 256, 3.5):
            with pytest.raises(ValueError):
                st.finish("ctg", 3, keys, min_quality=bad, draft=text)
        with pytest.raises(ValueError):
            st.finish("ctg", 3, keys, min_quality=20)
        assert st.finish("ctg", 3, keys, min_quality=0) == ungated == st.finish("ctg", 3, keys, min_quality=None)
        good(st, keys)


# ---- 6. the writers ----
def _host_files(pred, draft_fa, where, threads, **kw):
    perform_stitch(str(pred), str(where), threads, **kw)
    return gcases._files(where)


@pytest.mark.parametrize("fill", [False, True])
def test_stitch_directory_and_writers_write_the_host_files(planted, fill):
    pred, draft_fa, drafts, tmp = planted
    tag = "fill" if fill else "bare"
    kw = dict(qualities=True, edits=draft_fa, min_quality=20, draft=draft_fa)
    if fill:
        kw.update(fill=draft_fa, unpolished_contigs=True)
    host = _host_files(pred, draft_fa, tmp / ("host_" + tag) / "asm", 3, **kw)
    assert all(text for text in host) and len(host[3].splitlines()) == 8
    assert list(cases.fasta_sequences(host[0])) == (["b1", "ctg", "ctg2"] if fill else ["ctg"])
    assert [line.split("\t")[-1] for line in host[2].splitlines() if line.startswith("##")] == \
        (["withheld=0", "withheld=7", "withheld=0"] if fill else ["withheld=7"])
    stats = {}
    kw_dev = dict(kw)
    del kw_dev["qualities"]
    out = stitch_directory(str(pred), str(tmp / ("dev_" + tag) / "asm"), 3, stats=stats, qualities=True, **kw_dev)
    assert gcases._files(out[:-len(SUFFIXES[0])]) == host
    assert stats["gate"]["withheld"] == 7 and (stats["gate"]["sub"], stats["gate"]["del"], stats["gate"]["ins"]) == (3, 2, 2)
    assert stats["gate"]["bytes_returned"] == 7 * 16 and stats["gate"]["seconds"] > 0
    with DeviceStitcher(0) as st:
        ecases._feed(st, pred, "ctg", shuffle=3)
        st.write_fastq(str(tmp / ("writer_" + tag) / "asm"), 2 if fill else 3, **kw_dev)
        assert gcases._files(tmp / ("writer_" + tag) / "asm") == host
        # fewer files asked for: the same FASTA and the same .withheld.tsv
        bare = {k: v for k, v in kw_dev.items() if k != "edits"}
        st.write_fasta(str(tmp / ("fasta_" + tag) / "asm"), 2 if fill else 3, **bare)
        assert gcases._files(tmp / ("fasta_" + tag) / "asm") == (host[0], None, None, host[3])
        # and with the gate off the handle writes what it wrote before
        off = {k: v for k, v in kw_dev.items() if k not in ("min_quality", "draft")}
        st.write_fastq(str(tmp / ("off_" + tag) / "asm"), 3, min_quality=0, **off)
        assert gcases._files(tmp / ("off_" + tag) / "asm") == _host_files(pred, draft_fa, tmp / ("hostoff_" + tag) / "asm", 3,
                                                                         qualities=True, **off)
