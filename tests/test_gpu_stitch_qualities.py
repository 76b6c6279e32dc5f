"""The device stitch with qualities (pa_stitcher_add_qual / pa_stitcher_take_qualities through DeviceStitch.py) against
perform_stitch(..., qualities=True), the host form, on the same prediction files and the same `threads`: byte for byte the same
FASTA and the same FASTQ.  The host form itself is held to a literal restatement in tests/test_polish_qualities_cpu.py."""
import ctypes
import os

import numpy as np
import pytest

import test_polish_qualities_cpu as cases
from pepper_amd import _lib
from pepper_amd.polish.DataStorePredict import DataStore
from pepper_amd.polish.DeviceStitch import DeviceStitcher, stitch_directory, string_order_key
from test_polish_stitch import make_region

pytestmark = pytest.mark.gpu


def _device_texts(pred, where, threads, stats=None):
    out = stitch_directory(str(pred), str(where), threads, stats=stats, qualities=True)
    assert out == str(where) + "_pepper_polished.fa"
    return open(out).read(), open(str(where) + "_pepper_polished.fastq").read()


def _both(pred, tmp_path, threads, stats=None):
    """(FASTA, FASTQ) of the device, checked equal to the host's."""
    dev = _device_texts(pred, tmp_path / ("dev%d" % threads) / "asm", threads, stats)
    host = cases.host_texts(pred, tmp_path / ("host%d" % threads) / "asm", threads)
    assert dev == host
    cases.records(dev[1])
    return dev


def test_golden_inputs(golden_dir, tmp_path):
    cases.write_golden(golden_dir, tmp_path / "pred")
    want = open(os.path.join(golden_dir, "polish_stitch_ref.fa")).read()
    for threads in (1, 2):
        fasta, fastq = _both(tmp_path / "pred", tmp_path, threads)
        assert fasta == want and len(fastq) > len(fasta)


def test_rows_no_pipeline_would_write(tmp_path):
    cases.write_rows_no_pipeline_would_write(tmp_path / "pred")
    for threads in (1, 3):
        dev = _both(tmp_path / "pred", tmp_path, threads)
        assert dev == cases.expected_texts(tmp_path / "pred", threads) and len(dev[0]) > 1000


def test_later_write_wins_not_higher_phred(tmp_path):
    cases.write_one_key_twice(tmp_path / "a", 0, 1)
    assert _device_texts(tmp_path / "a", tmp_path / "oa", 1) == (">ctg\nC\n", "@ctg\nC\n+\n$\n")
    cases.write_one_key_twice(tmp_path / "b", 2, 10)
    assert _device_texts(tmp_path / "b", tmp_path / "ob", 1) == (">ctg\nA\n", "@ctg\nA\n+\n]\n")
    for name in ("a", "b"):
        assert _both(tmp_path / name, tmp_path / ("both_" + name), 1)


def test_gap_and_clamp(tmp_path):
    cases.write_gap_and_clamp(tmp_path / "pred")
    assert _both(tmp_path / "pred", tmp_path, 1) == (">ctg\nACGTA\n", "@ctg\nACGTA\n+\n!~~~~\n")


def test_empty_and_bad_labels(tmp_path):
    cases.write_empty_and_good(tmp_path / "pred")
    assert _both(tmp_path / "pred", tmp_path, 1) == (">c10\nTGCAT\n", "@c10\nTGCAT\n+\n\"#$%&\n")
    cases.write_bad_label(tmp_path / "bad")
    with pytest.raises(KeyError) as err:
        stitch_directory(str(tmp_path / "bad"), str(tmp_path / "ob"), 1, qualities=True)
    assert err.value.args[0] == 7
    assert open(str(tmp_path / "ob") + "_pepper_polished.fastq").read() == "@a\nACG\n+\n+5?\n"


def test_off_writes_no_fastq(tmp_path):
    cases.write_rows_no_pipeline_would_write(tmp_path / "pred")
    on = _device_texts(tmp_path / "pred", tmp_path / "on" / "asm", 3)
    out = stitch_directory(str(tmp_path / "pred"), str(tmp_path / "off" / "asm"), 3)
    assert open(out).read() == on[0] and os.listdir(os.path.dirname(out)) == ["asm_pepper_polished.fa"]


@pytest.mark.parametrize("size", ["B-1", "B", "B+1", "2B+1"])
def test_scan_boundaries(tmp_path, size):
    """The recipe of test_gpu_device_stitch.test_scan_boundaries: contig c2 has positions = slots = the size, contig c1 the same
    positions with an insert column behind a tenth of them and gaps among its labels, so a letter's place differs from its slot.
    Every row has its own phred: a quality one place off is seen."""
    B = DeviceStitcher.limits()["scan_block"]
    n = {"B-1": B - 1, "B": B, "B+1": B + 1, "2B+1": 2 * B + 1}[size]
    rng = np.random.default_rng(n)
    pred = tmp_path / "pred"
    pred.mkdir()
    rows = 700
    with DataStore(str(pred / "p.hdf"), "w") as s:
        pos = np.arange(n)
        for cid, at in enumerate(range(0, n, rows)):
            p = pos[at:at + rows]
            s.write_prediction("c2", 0, n, cid, p, np.zeros(len(p), np.int64), rng.integers(1, 5, len(p)), rng.integers(0, 120, len(p)))
        extra = pos[rng.random(n) < 0.1]
        ipos = np.concatenate([pos, extra])
        iidx = np.concatenate([np.zeros(n, np.int64), np.ones(len(extra), np.int64)])
        order = np.lexsort((iidx, ipos))
        ipos, iidx = ipos[order], iidx[order]
        for cid, at in enumerate(range(0, len(ipos), rows)):
            p = ipos[at:at + rows]
            s.write_prediction("c1", 0, n, cid, p, iidx[at:at + rows], rng.integers(0, 5, len(p)), rng.integers(0, 120, len(p)))
    stats = {}
    fasta, fastq = _both(pred, tmp_path, 1, stats)
    assert stats["slots"] == n and stats["positions"] == n          # (of the last contig finished: c2)
    recs = cases.records(fastq)
    assert [r[0] for r in recs] == ["c1", "c2"] and len(recs[1][1]) == n and len(recs[0][1]) < n + len(extra)
    assert (fasta, fastq) == cases.expected_texts(pred, 1)
    plain = {}
    stitch_directory(str(pred), str(tmp_path / "plain"), 1, stats=plain)
    assert stats["table_bytes"] == plain["table_bytes"] + n          # the quality buffer: one byte per letter


def test_insert_columns(tmp_path):
    """A region whose positions carry up to three insert columns (indices 0..3), next to an overlapping one."""
    rng = np.random.default_rng(77)
    pred = tmp_path / "pred"
    pred.mkdir()
    with DataStore(str(pred / "p.hdf"), "w") as s:
        for start, end in ((0, 1500), (1200, 2400)):
            pos = np.repeat(np.arange(start, end), rng.integers(1, 5, end - start))
            idx = np.concatenate([np.arange(k) for k in np.bincount(pos - start)])
            assert idx.max() == 3
            for cid, at in enumerate(range(0, len(pos), 950)):
                p, x = cases._padded(pos[at:at + 1000]), cases._padded(idx[at:at + 1000])
                s.write_prediction("ctg", start, end, cid, p, x, rng.integers(0, 5, 1000), rng.integers(0, 256, 1000))
    for threads in (1, 2):
        dev = _both(pred, tmp_path, threads)
        assert dev == cases.expected_texts(pred, threads) and len(dev[0]) > 3000


class _Capture(object):
    """A store that keeps what make_region writes and passes it on to a DataStore."""

    def __init__(self, store, path):
        self.store, self.path, self.chunks = store, path, []

    def write_prediction(self, contig, start, end, cid, position, index, bases, phred):
        self.chunks.append((contig, (self.path, "%s-%d-%d" % (contig, start, end), start, end), cid, np.asarray(position, np.int64),
                            np.asarray(index, np.int64), np.asarray(bases).astype(np.uint8), np.asarray(phred).astype(np.uint8)))
        self.store.write_prediction(contig, start, end, cid, position, index, bases, phred)


@pytest.fixture(scope="module")
def captured(tmp_path_factory):
    """Two contigs of three overlapping regions each, in one file and as arrays; the host's (sequence, quality) per contig for
    threads 1, 2 and 3."""
    tmp = tmp_path_factory.mktemp("stitch_qualities")
    rng = np.random.default_rng(5)
    pred = tmp / "pred"
    pred.mkdir()
    path = str(pred / "p.hdf")
    with DataStore(path, "w") as store:
        cap = _Capture(store, path)
        for contig in ("ctgA", "ctgB"):
            for start, end in ((0, 3000), (2000, 5000), (2500, 6000)):
                make_region(rng, cap, contig, start, end, 12)
    regions = {c: list(dict.fromkeys(k for cc, k, *_ in cap.chunks if cc == c)) for c in ("ctgA", "ctgB")}
    host = {}
    for threads in (1, 2, 3):
        _, fastq = cases.host_texts(pred, tmp / ("host%d" % threads), threads)
        recs = cases.records(fastq)
        assert [r[0] for r in recs] == ["ctgA", "ctgB"]
        host[threads] = {name: (seq, qual) for name, seq, qual in recs}
    assert host[1] != host[3]
    return cap.chunks, regions, host


def _add(st, part, device=False, with_phred=True, mixed=False):
    labels, phred = np.stack([c[5] for c in part]), np.stack([c[6] for c in part])
    if device:
        import torch
        labels = torch.from_numpy(labels).to("cuda:0")
        if not mixed:
            phred = torch.from_numpy(phred).to("cuda:0")
        torch.cuda.synchronize()
    st.add(part[0][0], [c[1] for c in part], [string_order_key(c[2]) for c in part], np.stack([c[3] for c in part]),
           np.stack([c[4] for c in part]), labels, phred if with_phred else None)


def test_arrival_order_does_not_matter(captured):
    """The shuffle of test_gpu_device_stitch.test_arrival_order_does_not_matter, with qualities: chunks of two contigs shuffled,
    interleaved, five per call, every other call with device tensors."""
    chunks, regions, host = captured
    order = np.random.default_rng(6).permutation(len(chunks)).tolist()
    with DeviceStitcher(0) as st:
        for a in range(0, len(order), 5):
            batch = [chunks[i] for i in order[a:a + 5]]
            for contig in ("ctgA", "ctgB"):
                part = [c for c in batch if c[0] == contig]
                if part:
                    _add(st, part, device=bool((a // 5) % 2))
        for threads in (1, 2):
            for contig in ("ctgA", "ctgB"):
                assert st.finish(contig, threads, regions[contig], qualities=True) == host[threads][contig]


def test_device_tensors_and_refinish(captured):
    """Labels and phred as device tensors against the same arrays on the host; a contig finished with threads 1, then 3, then 1
    gives each plan's own result; a device tensor beside a host array is refused."""
    chunks, regions, host = captured
    mine = [c for c in chunks if c[0] == "ctgA"]
    got = {}
    for device in (False, True):
        with DeviceStitcher(0) as st:
            for a in range(0, len(mine), 7):
                _add(st, mine[a:a + 7], device=device)
            held = st.stats()["rows"]
            with pytest.raises(ValueError):
                _add(st, mine[:3], device=True, mixed=True)
            assert st.stats()["rows"] == held
            got[device] = [st.finish("ctgA", threads, regions["ctgA"], qualities=True) for threads in (1, 3, 1)]
            assert st.finish("ctgA", 3, regions["ctgA"]) == host[3]["ctgA"][0]          # (a plain finish of the same rows)
    assert got[False] == got[True] == [host[1]["ctgA"], host[3]["ctgA"], host[1]["ctgA"]]


def test_missing_qualities(captured):
    chunks, regions, host = captured
    mine = [c for c in chunks if c[0] == "ctgB"]
    with DeviceStitcher(0) as st:
        _add(st, mine[:10])
        _add(st, mine[10:11], with_phred=False)
        _add(st, mine[11:])
        with pytest.raises(_lib.PepperAmdError) as err:
            st.finish("ctgB", 1, regions["ctgB"], qualities=True)
        assert err.value.code == _lib.PA_ERR_INVALID and "without qualities" in str(err.value)
        assert st.finish("ctgB", 1, regions["ctgB"]) == host[1]["ctgB"][0]
        assert st.finish("never added", 1, qualities=True) == ("", "")


def test_refusals(captured):
    chunks, regions, host = captured
    mine = [c for c in chunks if c[0] == "ctgA"]
    lib = _lib.load()
    with DeviceStitcher(0) as st:
        buf = ctypes.create_string_buffer(8)
        assert lib.pa_stitcher_take_qualities(st.handle, buf, 8) == _lib.PA_ERR_INVALID           # no finish yet
        assert b"finish" in lib.pa_last_error()
        _add(st, mine)
        sequence, quality = st.finish("ctgA", 1, regions["ctgA"], qualities=True)
        n = len(sequence)
        buf = ctypes.create_string_buffer(n)
        assert lib.pa_stitcher_take_qualities(st.handle, buf, n - 1) == _lib.PA_ERR_INVALID
        assert b"room for" in lib.pa_last_error()
        assert lib.pa_stitcher_take_qualities(st.handle, buf, n) == _lib.PA_OK and buf.raw[:n].decode() == quality
        assert (sequence, quality) == host[1]["ctgA"]
        assert st.finish("ctgA", 2, regions["ctgA"], qualities=True) == host[2]["ctgA"]
