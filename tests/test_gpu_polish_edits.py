"""The edit records of the device stitch (pa_stitcher_edits / pa_stitcher_take_edits through DeviceStitcher.edits) against the
numpy twin (pepper_amd/polish/Edits.records_numpy), record for record as bytes; the .edits.tsv of stitch_directory against
perform_stitch's, byte for byte; and the round trip Edits.apply(draft, records, pieces) == the consensus.  The twin itself is held
to a literal restatement in tests/test_polish_edits_cpu.py."""
import ctypes

import numpy as np
import pytest

import polish_edits_cases as cases
import test_polish_qualities_cpu as qcases
from pepper_amd import _lib, h5
from pepper_amd.polish import Edits
from pepper_amd.polish.DeviceStitch import DeviceStitcher, _read_region, stitch_directory
from pepper_amd.polish.perform_stitch import get_file_paths_from_directory

pytestmark = pytest.mark.gpu


def _feed(st, pred, contig, phred=True, shuffle=None, device=False):
    """Every chunk of the contig's prediction files to the stitcher, one add per chunk (shuffle: a seed for their order;
    device: every other add with device tensors).  -> the region keys."""
    keys, calls = [], []
    for fn in get_file_paths_from_directory(str(pred)):
        with h5.File(fn, 'r') as f:
            if 'predictions' not in f.keys() or contig not in f.keys('predictions'):
                continue
            for name, start, end in f.list_polish_regions(contig):
                key, at = (fn, name, start, end), 0
                keys.append(key)
                for block in _read_region(f, 'predictions/%s/%s-%d-%d' % (contig, contig, start, end), True):
                    for k in range(len(block[0])):
                        calls.append((key, at + k, [b[k:k + 1] for b in block]))
                    at += len(block[0])
    if shuffle is not None:
        calls = [calls[i] for i in np.random.default_rng(shuffle).permutation(len(calls))]
    for n, (key, order, (pos, idx, lab, phr)) in enumerate(calls):
        lab, phr = lab.astype(np.uint8), phr.astype(np.uint8)
        if device and n % 2:
            import torch
            lab, phr = torch.from_numpy(lab).to("cuda:0"), torch.from_numpy(phr).to("cuda:0")
            torch.cuda.synchronize()
        st.add(contig, [key], [order], pos, idx, lab, phr if phred else None)
    return keys


def _same(records, want):
    assert records.dtype == Edits.EDIT_DTYPE and len(records) == len(want)
    assert records.tobytes() == np.asarray(want, Edits.EDIT_DTYPE).tobytes()


def _check_files(pred, draft_fa, drafts, tmp, threads_list, **feed):
    """A prediction directory: records, pieces and sequence of every contig against the twin; the round trip; the .tsv."""
    for threads in threads_list:
        dev = stitch_directory(str(pred), str(tmp / ("dev%d" % threads) / "asm"), threads, edits=draft_fa)
        fasta, tsv = cases.host_texts(pred, draft_fa, tmp / ("host%d" % threads) / "asm", threads)
        assert open(dev).read() == fasta
        assert open(dev[:-3] + ".edits.tsv").read() == tsv
        for contig, sequence in cases.fasta_sequences(fasta).items():
            want_sequence, want, want_pieces = cases.host_records(pred, draft_fa, contig, threads)
            with DeviceStitcher(0) as st:
                keys = _feed(st, pred, contig, **feed)
                assert st.finish(contig, threads, keys) == want_sequence == sequence
                records = st.edits(drafts[contig])
                _same(records, want)
                assert st.pieces() == want_pieces
                assert st.last_edit_counts == [0] + [int((want["kind"] == k).sum()) for k in range(1, 6)]
            assert Edits.apply(drafts[contig], records, want_pieces) == sequence


@pytest.mark.parametrize("second_from", [170, 190])
def test_planted_cases(tmp_path, second_from):
    drafts = cases.write_planted(tmp_path / "pred", second_from)
    _check_files(tmp_path / "pred", cases.write_draft(tmp_path / "draft.fa", drafts), drafts, tmp_path, (1, 3))


def test_shuffled_split_adds_and_device_tensors(tmp_path):
    drafts = cases.write_planted(tmp_path / "pred")
    _check_files(tmp_path / "pred", cases.write_draft(tmp_path / "draft.fa", drafts), drafts, tmp_path, (3,), shuffle=8, device=True)


def test_golden_inputs(golden_dir, tmp_path):
    qcases.write_golden(golden_dir, tmp_path / "pred")
    drafts = cases.golden_draft(golden_dir)
    _check_files(tmp_path / "pred", cases.write_draft(tmp_path / "draft.fa", drafts), drafts, tmp_path, (1, 2))


# ---- one region fed from arrays: the sizes the scans turn at ----
KEY = ("memory", "c-0-0", 0, 0)


def _add_rows(st, contig, table, chunk=61, phred=True):
    """{(position, index): (label, phred)} as chunks of `chunk` rows, the last one padded with (-1, -1)."""
    keys = sorted(table)
    n = (len(keys) + chunk - 1) // chunk
    pos, idx = -np.ones((n, chunk), np.int64), -np.ones((n, chunk), np.int64)
    lab, phr = np.zeros((n, chunk), np.uint8), np.zeros((n, chunk), np.uint8)
    for k, (p, i) in enumerate(keys):
        pos[k // chunk, k % chunk], idx[k // chunk, k % chunk] = p, i
        lab[k // chunk, k % chunk], phr[k // chunk, k % chunk] = table[(p, i)]
    st.add(contig, [KEY] * n, list(range(n)), pos, idx, lab, phr if phred else None)


def _twin(table, draft, phred=True):
    keys = sorted(table)
    return Edits.records_numpy([k[0] for k in keys], [k[1] for k in keys], [table[k][0] for k in keys],
                               [table[k][1] for k in keys] if phred else None, draft)


def _table(draft, a, b, phred=40):
    return {(p, 0): (cases.CODE[draft[p]], phred) for p in range(a, b)}


def _run(table, draft, phred=True):
    """-> (sequence, records, stats) of one stitcher; the records are the twin's, the round trip holds."""
    with DeviceStitcher(0) as st:
        _add_rows(st, "c", table, phred=phred)
        sequence = st.finish("c", 1, [KEY])
        before = st.stats()
        records = st.edits(draft)
        stats = st.stats()
        pieces = st.pieces()
    _same(records, _twin(table, draft, phred))
    assert stats["table_bytes"] == before["table_bytes"] + 16 * len(records)          # the record buffer and nothing else
    assert {k: v for k, v in stats.items() if k != "table_bytes"} == {k: v for k, v in before.items() if k != "table_bytes"}
    assert Edits.apply(draft, records, pieces) == sequence
    return sequence, records, stats


@pytest.mark.parametrize("edits", ["0", "1", "B-1", "B", "B+1", "2B+1"])
def test_edit_counts_at_the_scan_block(edits):
    """A contig of 2 B + 400 positions with exactly that many records, of all five kinds, spread over the whole of it."""
    B = DeviceStitcher.limits()["scan_block"]
    assert B == 1024
    n = {"0": 0, "1": 1, "B-1": B - 1, "B": B, "B+1": B + 1, "2B+1": 2 * B + 1}[edits]
    rng = np.random.default_rng(n)
    size = 2 * B + 400
    draft = cases.random_draft(rng, size)
    table = _table(draft, 0, size)
    left = n
    if left >= 2:                                                    # one uncovered position: GAP_OPEN + GAP_CLOSE
        del table[(size // 2, 0)]
        left -= 2
    spots = rng.permutation(np.delete(np.arange(1, size - 1), [size // 2 - 1]))[:left]
    for k, p in enumerate(spots.tolist()):
        if k % 3 == 0:
            table[(p, 0)] = (cases.other(draft[p]), k % 256)
        elif k % 3 == 1:
            table[(p, 0)] = (0, k % 256)
        else:
            table[(p, 1)] = (1 + k % 4, k % 256)
    _, records, stats = _run(table, draft)
    assert len(records) == n and stats["slots"] > 2 * B


@pytest.mark.parametrize("slots", ["B-1", "B", "B+1"])
def test_slot_counts_at_the_scan_block(slots):
    """As many slots as a workgroup of the scans takes, one fewer and one more, with an edit in the first and in the last slot."""
    B = DeviceStitcher.limits()["scan_block"]
    n = {"B-1": B - 1, "B": B, "B+1": B + 1}[slots]
    draft = cases.random_draft(np.random.default_rng(n), n + 7)
    table = _table(draft, 5, 5 + n)
    table[(5, 0)] = (cases.other(draft[5]), 1)
    table[(4 + n, 0)] = (0, 2)
    _, records, stats = _run(table, draft)
    assert stats["slots"] == n and [(int(r["position"]), int(r["kind"])) for r in records] == [(5, 1), (4 + n, 2)]
    assert [int(r["offset"]) for r in records] == [0, n - 1]


def test_insert_columns_and_one_deep_position():
    """Insert indices up to 3 all over, and one position with 300 insert slots (some empty, some gaps) in front of a gap run."""
    rng = np.random.default_rng(31)
    draft = cases.random_draft(rng, 900)
    table = _table(draft, 0, 900)
    for p in range(0, 900, 3):
        for i in range(1, int(rng.integers(1, 5))):
            table[(p, i)] = (int(rng.integers(0, 5)), int(rng.integers(0, 256)))
    for i in range(1, 301):
        if i % 7:
            table[(450, i)] = (int(rng.integers(0, 5)), i % 256)
    for p in range(451, 460):
        for i in range(4):
            table.pop((p, i), None)
    _, records, stats = _run(table, draft)
    assert int(records["index"].max()) == 300 and stats["slots"] > 1500
    at = records[records["position"] == 450]
    assert len(at) > 150 and (records["kind"] == 4).sum() == 1 and records[records["kind"] == 4]["position"][0] == 451


def test_without_qualities(tmp_path):
    """A contig added without phred: every record's phred is 0 and the text has '.' for min_phred."""
    rng = np.random.default_rng(3)
    draft = cases.random_draft(rng, 300)
    table = _table(draft, 0, 300, phred=77)
    table[(10, 0)] = (cases.other(draft[10]), 90)
    table[(20, 1)] = (2, 91)
    table[(30, 0)] = (0, 92)
    _, records, _ = _run(table, draft, phred=False)
    assert len(records) == 3 and not records["phred"].any()
    draft_fa = cases.write_draft(tmp_path / "draft.fa", {"c": draft})
    with DeviceStitcher(0) as st:
        _add_rows(st, "c", table, phred=False)
        st.write_fasta(str(tmp_path / "asm"), 1, edits=draft_fa)
    lines = open(str(tmp_path / "asm") + "_pepper_polished.edits.tsv").read().splitlines()
    assert [line.split("\t")[-1] for line in lines[1:4]] == [".", ".", "."] and len(lines) == 5
    with DeviceStitcher(0) as st:
        _add_rows(st, "c", table, phred=True)
        st.write_fastq(str(tmp_path / "q"), 1, edits=draft_fa)
    lines = open(str(tmp_path / "q") + "_pepper_polished.edits.tsv").read().splitlines()
    assert [line.split("\t")[-1] for line in lines[1:4]] == ["90", "91", "92"]


def test_refinish_and_two_runs(tmp_path):
    """One handle finished with threads 1, 3, 1: the edits asked for after each finish are that plan's; a second handle gives the
    same bytes."""
    drafts = cases.write_planted(tmp_path / "pred")
    draft_fa = cases.write_draft(tmp_path / "draft.fa", drafts)
    want = {t: cases.host_records(tmp_path / "pred", draft_fa, "ctg", t) for t in (1, 3)}
    assert want[1][1].tobytes() != want[3][1].tobytes()
    runs = []
    for _ in range(2):
        got = []
        with DeviceStitcher(0) as st:
            keys = _feed(st, tmp_path / "pred", "ctg")
            for threads in (1, 3, 1):
                assert st.finish("ctg", threads, keys) == want[threads][0]
                records = st.edits(drafts["ctg"])
                _same(records, want[threads][1])
                counted = st.stats()["table_bytes"]
                _same(st.edits(drafts["ctg"]), want[threads][1])     # asked twice: the same records, counted once
                assert st.stats()["table_bytes"] == counted
                got.append(records.tobytes())
        runs.append(got)
    assert runs[0] == runs[1]


def test_refusals_leave_the_handle_usable(tmp_path):
    drafts = cases.write_planted(tmp_path / "pred")
    draft_fa = cases.write_draft(tmp_path / "draft.fa", drafts)
    draft = drafts["ctg"].encode()
    _, want, _ = cases.host_records(tmp_path / "pred", draft_fa, "ctg", 3)
    lib = _lib.load()
    n, counts = ctypes.c_int64(), (ctypes.c_int64 * 6)()
    buf = np.zeros(len(want) + 1, Edits.EDIT_DTYPE)

    def edits(st, text=draft):
        return lib.pa_stitcher_edits(st.handle, text, len(text), ctypes.byref(n), counts)

    def good(st, keys):
        assert st.finish("ctg", 3, keys) and edits(st) == _lib.PA_OK and n.value == len(want)
        assert lib.pa_stitcher_take_edits(st.handle, buf.ctypes.data, n.value) == _lib.PA_OK
        _same(buf[:n.value], want)

    with DeviceStitcher(0) as st:
        assert edits(st) == _lib.PA_ERR_INVALID and b"no contig has been finished" in lib.pa_last_error()
        assert lib.pa_stitcher_take_edits(st.handle, buf.ctypes.data, len(buf)) == _lib.PA_ERR_INVALID
        keys = _feed(st, tmp_path / "pred", "ctg")
        st.finish("ctg", 3, keys)
        assert lib.pa_stitcher_take_edits(st.handle, buf.ctypes.data, len(buf)) == _lib.PA_ERR_INVALID        # no edits yet
        assert b"has not run" in lib.pa_last_error()
        assert edits(st, draft[:350]) == _lib.PA_ERR_INVALID and b"350" in lib.pa_last_error()                # piece_last = 350
        assert edits(st, draft[:351]) == _lib.PA_OK and n.value == len(want)
        assert lib.pa_stitcher_take_edits(st.handle, buf.ctypes.data, n.value - 1) == _lib.PA_ERR_INVALID
        assert b"room for" in lib.pa_last_error()
        good(st, keys)
        # a finish that gives no sequence: a label that is no base
        st.add("bad", [KEY], [0], np.arange(4).reshape(1, 4), np.zeros((1, 4), np.int64), np.array([[1, 7, 2, 3]], np.uint8),
               np.zeros((1, 4), np.uint8))
        with pytest.raises(KeyError):
            st.finish("bad", 1, [KEY])
        assert edits(st) == _lib.PA_ERR_INVALID and b"no sequence" in lib.pa_last_error()
        assert lib.pa_stitcher_take_edits(st.handle, buf.ctypes.data, len(buf)) == _lib.PA_ERR_INVALID        # that finish invalidated them
        good(st, keys)
        # a finish with more pieces than a record names: every region in piece 0 of 65 536
        contig_id, ids, _ = st._contigs["ctg"]
        region = np.array(list(ids.values()), np.int32)
        piece, rank = np.zeros(len(region), np.int32), np.arange(len(region), dtype=np.int64)
        first, last, length = (np.empty(65536, np.int64) for _ in range(3))
        total, bad = ctypes.c_int64(), ctypes.c_int32()
        assert lib.pa_stitcher_finish(st.handle, contig_id, len(region), region.ctypes.data, piece.ctypes.data, rank.ctypes.data, 65536,
                                      first.ctypes.data, last.ctypes.data, length.ctypes.data, ctypes.byref(total),
                                      ctypes.byref(bad)) == _lib.PA_OK and total.value > 0
        assert edits(st) == _lib.PA_ERR_INVALID and b"65536 pieces" in lib.pa_last_error()
        good(st, keys)
