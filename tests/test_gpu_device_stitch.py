"""The device stitch (pepper_amd/csrc/stitch.hip through pepper_amd/polish/DeviceStitch.py) against perform_stitch, the pinned
host path, on the same prediction files and the same `threads`: byte for byte the same FASTA."""
import os

import numpy as np
import pytest

from pepper_amd import _lib
from pepper_amd.polish import Stitch
from pepper_amd.polish.DataStorePredict import DataStore
from pepper_amd.polish.DeviceStitch import DeviceStitcher, stitch_directory, string_order_key
from pepper_amd.polish.perform_stitch import perform_stitch
from test_polish_stitch import dict_stitch, make_region

pytestmark = pytest.mark.gpu


def _both(pred, tmp_path, threads, tag=""):
    """(device FASTA text, host FASTA text) of one prediction directory."""
    dev = stitch_directory(str(pred), str(tmp_path / ("dev%s%d" % (tag, threads)) / "asm"), threads)
    host = perform_stitch(str(pred), str(tmp_path / ("host%s%d" % (tag, threads)) / "asm"), threads)
    assert dev.endswith("asm_pepper_polished.fa")
    return open(dev).read(), open(host).read()


def test_reference_golden(golden_dir, tmp_path):
    """polish_stitch_inputs.npz -> polish_stitch_ref.fa, the reference's own output."""
    g = np.load(os.path.join(golden_dir, "polish_stitch_inputs.npz"), allow_pickle=False)
    pred = tmp_path / "pred"
    pred.mkdir()
    stores = [DataStore(str(pred / ("pepper_prediction_%d.hdf" % i)), "w") for i in range(2)]
    for ri in range(int(g["n_regions"])):
        fi, start, end, n_chunks = (int(v) for v in g["r%d_meta" % ri])
        contig = str(g["r%d_contig" % ri])
        for cid in range(n_chunks):
            stores[fi].write_prediction(contig, start, end, cid, g["r%d_c%d_position" % (ri, cid)], g["r%d_c%d_index" % (ri, cid)],
                                        g["r%d_c%d_bases" % (ri, cid)], g["r%d_c%d_phred" % (ri, cid)])
    for s in stores:
        s.close()
    want = open(os.path.join(golden_dir, "polish_stitch_ref.fa")).read()
    for threads in (1, 2):
        dev, host = _both(pred, tmp_path, threads)
        assert dev == want and host == want


def test_rows_no_pipeline_would_write(tmp_path):
    """The recipe of test_native_merge_on_rows_no_pipeline_would_write: an unsorted chunk, a key twice in one chunk, in two chunks,
    in two regions and in two files, odd-length chunks, a region landing before everything merged so far, -1 positions and indices."""
    pred = tmp_path / "pred"
    pred.mkdir()
    files = [str(pred / "p0.hdf"), str(pred / "p1.hdf")]
    r = np.random.default_rng(22)
    with DataStore(files[0], "w") as a, DataStore(files[1], "w") as b:
        for store, start, end in ((a, 3000, 4000), (b, 0, 2500), (a, 2400, 3300), (b, 3000, 4000)):     # (3000, 4000) in both files
            for cid in range(3):
                n = int(r.integers(5, 400)) if cid == 1 else 1000
                pos = r.integers(start, end + 300, n)
                pos[r.random(n) < 0.05] = -1
                idx = r.integers(-1, 3, n)
                if cid != 2:
                    order = np.lexsort((idx, pos))
                    pos, idx = pos[order], idx[order]
                store.write_prediction("ctg", start, end, cid, pos, idx, r.integers(0, 5, n), np.zeros(n))
    for threads in (1, 3):
        dev, host = _both(pred, tmp_path, threads)
        assert dev == host and dev.splitlines()[1] == dict_stitch(files, "ctg", threads) and len(dev) > 1000


def test_chunk_ids_in_string_order(tmp_path):
    rng = np.random.default_rng(31)
    pred = tmp_path / "pred"
    pred.mkdir()
    path = str(pred / "p.hdf")
    with DataStore(path, "w") as store:
        for start, end in ((0, 900), (700, 1600)):
            for cid in range(12):
                n = 150
                pos = np.sort(rng.integers(start, end, n))
                idx = rng.integers(0, 2, n)
                order = np.lexsort((idx, pos))
                store.write_prediction("ctg", start, end, cid, pos[order], idx[order], rng.integers(1, 5, n), np.zeros(n))
    dev, host = _both(pred, tmp_path, 1)
    assert dev == host and dev.splitlines()[1] == dict_stitch([path], "ctg", 1) and len(dev) > 500


def test_keys_in_two_pieces_appear_twice(tmp_path):
    """Pieces are never merged with each other: three overlapping regions of one contig in one file give 5 909 letters as one
    piece (threads = 1) and 7 745 as two (threads = 2, 3)."""
    rng = np.random.default_rng(5)
    pred = tmp_path / "pred"
    pred.mkdir()
    path = str(pred / "p.hdf")
    with DataStore(path, "w") as store:
        for start, end in ((0, 3000), (2000, 5000), (2500, 6000)):
            make_region(rng, store, "ctg", start, end, 12)
    lengths = {}
    for threads in (1, 2, 3):
        dev, host = _both(pred, tmp_path, threads)
        assert dev == host and dev.splitlines()[1] == dict_stitch([path], "ctg", threads)
        lengths[threads] = len(dev.splitlines()[1])
    assert lengths[2] > lengths[1]
    assert lengths == {1: 5909, 2: 7745, 3: 7745}


def test_empty_results_and_bad_labels(tmp_path):
    pred = tmp_path / "pred"
    pred.mkdir()
    with DataStore(str(pred / "p.hdf"), "w") as s:
        s.write_prediction("c1", 0, 1000, 0, np.arange(1000), np.zeros(1000, dtype=np.int64), np.zeros(1000), np.zeros(1000))
        s.write_prediction("c2", 0, 10, 0, -np.ones(1000, dtype=np.int64), -np.ones(1000, dtype=np.int64), np.ones(1000), np.zeros(1000))
    dev, host = _both(pred, tmp_path, 1)
    assert dev == "" and host == ""           # an all-gap contig and a padding-only contig write nothing

    labels = np.array([1, 2, 3, 4, 0, 7, 1, 1, 1, 1])
    bad = tmp_path / "bad"
    bad.mkdir()
    with DataStore(str(bad / "p.hdf"), "w") as s:
        s.write_prediction("c", 0, 10, 0, np.arange(10), np.zeros(10, np.int64), labels, np.zeros(10))
    with pytest.raises(KeyError):
        perform_stitch(str(bad), str(tmp_path / "bad_host"), 1)
    with pytest.raises(KeyError) as err:
        stitch_directory(str(bad), str(tmp_path / "bad_dev"), 1)
    assert err.value.args[0] == 7

    over = tmp_path / "over"                  # the 7 is overwritten by chunk "1": nothing to raise
    over.mkdir()
    with DataStore(str(over / "p.hdf"), "w") as s:
        s.write_prediction("c", 0, 10, 0, np.arange(10), np.zeros(10, np.int64), labels, np.zeros(10))
        s.write_prediction("c", 0, 10, 1, np.arange(4, 7), np.zeros(3, np.int64), np.array([2, 3, 0]), np.zeros(3))
    dev, host = _both(over, tmp_path, 1, "over")
    assert dev == host == ">c\nACGTCGAAA\n"


SCAN_BLOCK = None


def _scan_block():
    global SCAN_BLOCK
    if SCAN_BLOCK is None:
        SCAN_BLOCK = DeviceStitcher.limits()["scan_block"]
    return SCAN_BLOCK


@pytest.mark.parametrize("size", ["B-1", "B", "B+1", "2B+1", "B*B+1"])
def test_scan_boundaries(tmp_path, size):
    """Both scans (widths over the positions, letters over the slots) at the sizes where the number of block sums changes level:
    contig c2 starts at 0 with every index 0, so positions = slots = the size; contig c1 has the same positions with inserts and
    gaps, so its slots and letters differ from its positions.  Checked against the numpy form of the host merge."""
    B = _scan_block()
    n = {"B-1": B - 1, "B": B, "B+1": B + 1, "2B+1": 2 * B + 1, "B*B+1": B * B + 1}[size]
    rng = np.random.default_rng(n % 1000)
    pred = tmp_path / "pred"
    pred.mkdir()
    path = str(pred / "p.hdf")
    rows = 60000                               # rows per chunk (not the pipeline's 1000: fewer, larger datasets)
    with DataStore(path, "w") as s:
        pos = np.arange(n)
        for cid, at in enumerate(range(0, n, rows)):
            p = pos[at:at + rows]
            s.write_prediction("c2", 0, n, cid, p, np.zeros(len(p), np.int64), rng.integers(1, 5, len(p)), np.zeros(len(p)))
        extra = pos[rng.random(n) < 0.1]       # an insert column behind a tenth of the positions
        ipos = np.concatenate([pos, extra])
        iidx = np.concatenate([np.zeros(n, np.int64), np.ones(len(extra), np.int64)])
        order = np.lexsort((iidx, ipos))
        ipos, iidx = ipos[order], iidx[order]
        for cid, at in enumerate(range(0, len(ipos), rows)):
            p = ipos[at:at + rows]
            s.write_prediction("c1", 0, n, cid, p, iidx[at:at + rows], rng.integers(0, 5, len(p)), np.zeros(len(p)))
    stats = {}
    out = stitch_directory(str(pred), str(tmp_path / "dev"), 1, stats=stats)
    assert stats["slots"] == n and stats["positions"] == n          # (of the last contig finished: c2)
    assert stats["rows"] == 2 * n + len(extra)
    lines = open(out).read().splitlines()
    assert lines[0::2] == [">c1", ">c2"]
    for name, seq in zip(("c1", "c2"), lines[1::2]):
        first, last, want = Stitch.small_chunk_stitch_numpy(name, [(path, name, 0, n)])
        assert (first, last) == (0, n - 1) and seq == want
    assert len(lines[3]) == n and len(lines[1]) < n + len(extra)


class _Capture(object):
    """A store that keeps what make_region writes and passes it on to a DataStore."""

    def __init__(self, store, path):
        self.store, self.path, self.chunks = store, path, []

    def write_prediction(self, contig, start, end, cid, position, index, bases, phred):
        self.chunks.append((contig, (self.path, "%s-%d-%d" % (contig, start, end), start, end), cid, np.asarray(position, np.int64),
                            np.asarray(index, np.int64), np.asarray(bases).astype(np.uint8)))
        self.store.write_prediction(contig, start, end, cid, position, index, bases, phred)


def test_arrival_order_does_not_matter(tmp_path):
    """Through DeviceStitcher directly: the chunks of two contigs shuffled, interleaved, split over several add calls, half of the
    labels on the device and half on the host, give the strings perform_stitch gives; an insert index of 65 536 (or a position of
    2^32) is refused loudly and leaves the handle as it was."""
    import torch
    rng = np.random.default_rng(5)
    pred = tmp_path / "pred"
    pred.mkdir()
    path = str(pred / "p.hdf")
    with DataStore(path, "w") as store:
        cap = _Capture(store, path)
        for contig in ("ctgA", "ctgB"):
            for start, end in ((0, 3000), (2000, 5000), (2500, 6000)):
                make_region(rng, cap, contig, start, end, 12)
    regions = {c: list(dict.fromkeys(k for cc, k, *_ in cap.chunks if cc == c)) for c in ("ctgA", "ctgB")}
    order = rng.permutation(len(cap.chunks)).tolist()
    with DeviceStitcher(0) as st:
        for a in range(0, len(order), 5):
            batch = [cap.chunks[i] for i in order[a:a + 5]]
            for contig in ("ctgA", "ctgB"):
                part = [c for c in batch if c[0] == contig]
                if not part:
                    continue
                labels = np.stack([c[5] for c in part])
                if (a // 5) % 2:
                    labels = torch.from_numpy(labels).to("cuda:0")
                    torch.cuda.synchronize()
                st.add(contig, [c[1] for c in part], [string_order_key(c[2]) for c in part], np.stack([c[3] for c in part]),
                       np.stack([c[4] for c in part]), labels)
        held = st.stats()["rows"]
        key = regions["ctgA"][0]
        row = np.zeros((1, 1000), np.int64)
        for position, index in ((row + 5, row + 65536), (row + 2 ** 32, row)):
            with pytest.raises(_lib.PepperAmdError) as err:
                st.add("ctgA", [key], [string_order_key(99)], position, index, np.ones((1, 1000), np.uint8))
            assert err.value.code == _lib.PA_ERR_UNSUPPORTED
        assert st.stats()["rows"] == held
        # a row the merge drops anyway may hold anything
        st.add("ctgA", [key], [string_order_key(99)], row - 1, row + 65536, np.ones((1, 1000), np.uint8))
        assert st.stats()["rows"] == held
        for threads in (1, 2):
            host = open(perform_stitch(str(pred), str(tmp_path / ("host%d" % threads)), threads)).read().splitlines()
            assert host[0::2] == [">ctgA", ">ctgB"]
            for contig, want in zip(("ctgA", "ctgB"), host[1::2]):
                assert st.finish(contig, threads, regions[contig]) == want
