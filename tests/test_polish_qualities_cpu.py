"""perform_stitch(..., qualities=True): the FASTQ beside the FASTA, held byte for byte to a literal restatement written here --
the dictionary merge of test_polish_stitch.dict_stitch with the value (label, phred): per piece a dict keyed (position, insert
index), later writes overwrite, a winning gap emits nothing, a letter's quality is chr(33 + min(phred, 93)) of the write that
won.  No GPU.  The builders below also feed tests/test_gpu_stitch_qualities.py."""
import inspect
import os

import numpy as np
import pytest

from pepper_amd import _lib, h5
from pepper_amd.polish.DataStorePredict import DataStore
from pepper_amd.polish.perform_stitch import natural_key, perform_stitch

DECODE = {1: 'A', 2: 'C', 3: 'G', 4: 'T', 0: ''}


def dict_stitch_q(pred_files, contig, threads=1):
    """Literal restatement -> (sequence, quality)."""
    keys = []
    for fn in pred_files:
        with h5.File(fn) as f:
            if contig not in f.keys('predictions'):
                continue
            for ck in sorted(f.keys('predictions/' + contig)):
                keys.append((fn, ck, int(f[f'predictions/{contig}/{ck}/contig_start']), int(f[f'predictions/{contig}/{ck}/contig_end'])))
    keys = sorted(sorted(keys, key=lambda e: e[1]), key=lambda e: (e[2], e[3]))
    size = max(2, int(len(keys) / threads) + 1)
    pieces = []
    for i in range(0, len(keys), size):
        table = {}
        for fn, ck, st, en in keys[i:i + size]:
            with h5.File(fn) as f:
                for cid in sorted(set(f.keys(f'predictions/{contig}/{ck}')) - {'contig_start', 'contig_end'}):
                    base = f'predictions/{contig}/{ck}/{cid}/'
                    for pos, idx, b, q in zip(f[base + 'position'].tolist(), f[base + 'index'].tolist(), f[base + 'bases'].tolist(),
                                              f[base + 'phred_score'].tolist()):
                        if st > 0 and pos <= st + 200:
                            continue
                        if idx < 0 or pos < 0:
                            continue
                        table[(pos, idx)] = (b, q)
        if table:
            order = sorted(table)
            letters = [DECODE[table[k][0]] for k in order]           # KeyError(label) as label_decoder raises it
            quality = [chr(33 + min(table[k][1], 93)) for k, letter in zip(order, letters) if letter]
            pieces.append((order[0][0], order[-1][0], ''.join(letters), ''.join(quality)))
    pieces.sort(key=lambda e: (e[0], e[1]))
    return ''.join(p[2] for p in pieces), ''.join(p[3] for p in pieces)


def expected_files(pred):
    files = sorted(os.path.join(pred, f) for f in os.listdir(pred) if f.endswith("hdf"))
    contigs = set()
    for fn in files:
        with h5.File(fn) as f:
            contigs.update(f.keys('predictions'))
    return files, sorted(contigs, key=natural_key)


def expected_texts(pred, threads):
    """(FASTA text, FASTQ text) of a prediction directory by the restatement."""
    files, contigs = expected_files(str(pred))
    fasta, fastq = "", ""
    for contig in contigs:
        seq, qual = dict_stitch_q(files, contig, threads)
        if seq:
            fasta += ">" + contig + "\n" + seq + "\n"
            fastq += "@" + contig + "\n" + seq + "\n+\n" + qual + "\n"
    return fasta, fastq


def records(fastq_text):
    lines = fastq_text.splitlines()
    assert len(lines) % 4 == 0
    out = []
    for k in range(0, len(lines), 4):
        assert lines[k][0] == "@" and lines[k + 2] == "+" and len(lines[k + 3]) == len(lines[k + 1])
        out.append((lines[k][1:], lines[k + 1], lines[k + 3]))
    return out


def host_texts(pred, where, threads):
    out = perform_stitch(str(pred), str(where), threads, qualities=True)
    assert out == str(where) + "_pepper_polished.fa"
    return open(out).read(), open(str(where) + "_pepper_polished.fastq").read()


# ---- the inputs (shared with the GPU tests) ----
def write_golden(golden_dir, pred):
    g = np.load(os.path.join(golden_dir, "polish_stitch_inputs.npz"), allow_pickle=False)
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


def write_rows_no_pipeline_would_write(pred):
    """The recipe of test_rows_no_pipeline_would_write with a phred from 0..255 per row: unsorted chunks, a key twice in a chunk, in
    two chunks, in two regions and in two files, odd-length chunks, -1 rows."""
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
                store.write_prediction("ctg", start, end, cid, pos, idx, r.integers(0, 5, n), r.integers(0, 256, n))
    return files


def _padded(values, fill=-1, length=1000):
    out = np.full(length, fill, np.int64)
    out[:len(values)] = values
    return out


def write_one_key_twice(pred, earlier_id, later_id):
    """Key (5, 0) written by two chunks of one region: label 1 / phred 60 under `earlier_id`, label 2 / phred 3 under `later_id`
    (rows of the pipeline's length, padded with -1)."""
    pred.mkdir()
    with DataStore(str(pred / "p.hdf"), "w") as s:
        for cid, label, phred in ((earlier_id, 1, 60), (later_id, 2, 3)):
            s.write_prediction("ctg", 0, 10, cid, _padded([5]), _padded([0]), _padded([label], 0), _padded([phred], 0))


def write_gap_and_clamp(pred):
    """Chunk 0 writes a base at positions 0..5; chunk 1 overwrites position 0 with a gap and positions 1..5 with phred 0, 93, 94,
    100, 255 (short chunks: read dataset by dataset)."""
    pred.mkdir()
    with DataStore(str(pred / "p.hdf"), "w") as s:
        s.write_prediction("ctg", 0, 10, 0, np.arange(6), np.zeros(6, np.int64), np.full(6, 3), np.full(6, 40))
        s.write_prediction("ctg", 0, 10, 1, np.arange(6), np.zeros(6, np.int64), np.array([0, 1, 2, 3, 4, 1]),
                           np.array([77, 0, 93, 94, 100, 255]))


def write_empty_and_good(pred):
    """c1: gaps only; c2: padding only; c10: five bases."""
    pred.mkdir()
    with DataStore(str(pred / "p.hdf"), "w") as s:
        s.write_prediction("c1", 0, 1000, 0, np.arange(1000), np.zeros(1000, np.int64), np.zeros(1000), np.full(1000, 9))
        s.write_prediction("c2", 0, 10, 0, -np.ones(1000, np.int64), -np.ones(1000, np.int64), np.ones(1000), np.full(1000, 9))
        s.write_prediction("c10", 0, 10, 0, np.arange(5), np.zeros(5, np.int64), np.array([4, 3, 2, 1, 4]), np.array([1, 2, 3, 4, 5]))


def write_bad_label(pred):
    """Contig a is fine; contig c keeps a label 7."""
    pred.mkdir()
    with DataStore(str(pred / "p.hdf"), "w") as s:
        s.write_prediction("a", 0, 10, 0, np.arange(3), np.zeros(3, np.int64), np.array([1, 2, 3]), np.array([10, 20, 30]))
        s.write_prediction("c", 0, 10, 0, np.arange(10), np.zeros(10, np.int64), np.array([1, 2, 3, 4, 0, 7, 1, 1, 1, 1]), np.full(10, 12))


# ---- the cases ----
def test_golden_inputs(golden_dir, tmp_path):
    pred = tmp_path / "pred"
    write_golden(golden_dir, pred)
    want = open(os.path.join(golden_dir, "polish_stitch_ref.fa")).read()
    for threads in (1, 2):
        fasta, fastq = host_texts(pred, tmp_path / ("o%d" % threads) / "asm", threads)
        assert fasta == want
        assert (fasta, fastq) == expected_texts(pred, threads)
        recs, lines = records(fastq), fasta.splitlines()
        assert recs and [(name, seq) for name, seq, _ in recs] == [(lines[k][1:], lines[k + 1]) for k in range(0, len(lines), 2)]
        assert all(len(q) == len(s) for _, s, q in recs)


def test_rows_no_pipeline_would_write(tmp_path):
    pred = tmp_path / "pred"
    write_rows_no_pipeline_would_write(pred)
    for threads in (1, 3):
        fasta, fastq = host_texts(pred, tmp_path / ("o%d" % threads), threads)
        assert (fasta, fastq) == expected_texts(pred, threads)
        (name, seq, qual), = records(fastq)
        assert name == "ctg" and len(seq) > 1000 and "~" in qual and len(set(qual)) > 60


def test_later_write_wins_not_higher_phred(tmp_path):
    write_one_key_twice(tmp_path / "a", 0, 1)
    fasta, fastq = host_texts(tmp_path / "a", tmp_path / "oa", 1)
    assert fasta == ">ctg\nC\n" and fastq == "@ctg\nC\n+\n$\n"
    assert (fasta, fastq) == expected_texts(tmp_path / "a", 1)
    # "10" sorts before "2": the chunk written as the later one is now the earlier one
    write_one_key_twice(tmp_path / "b", 2, 10)
    fasta, fastq = host_texts(tmp_path / "b", tmp_path / "ob", 1)
    assert fasta == ">ctg\nA\n" and fastq == "@ctg\nA\n+\n]\n"
    assert (fasta, fastq) == expected_texts(tmp_path / "b", 1)


def test_gap_and_clamp(tmp_path):
    write_gap_and_clamp(tmp_path / "pred")
    fasta, fastq = host_texts(tmp_path / "pred", tmp_path / "o", 1)
    assert fasta == ">ctg\nACGTA\n" and fastq == "@ctg\nACGTA\n+\n!~~~~\n"
    assert (fasta, fastq) == expected_texts(tmp_path / "pred", 1)


def test_empty_and_bad_labels(tmp_path):
    write_empty_and_good(tmp_path / "pred")
    fasta, fastq = host_texts(tmp_path / "pred", tmp_path / "o", 1)
    assert fasta == ">c10\nTGCAT\n" and fastq == "@c10\nTGCAT\n+\n\"#$%&\n"
    assert (fasta, fastq) == expected_texts(tmp_path / "pred", 1)

    write_bad_label(tmp_path / "bad")
    with pytest.raises(KeyError) as err:
        dict_stitch_q([str(tmp_path / "bad" / "p.hdf")], "c")
    assert err.value.args[0] == 7
    with pytest.raises(KeyError) as err:
        perform_stitch(str(tmp_path / "bad"), str(tmp_path / "ob"), 1, qualities=True)
    assert err.value.args[0] == 7
    assert open(str(tmp_path / "ob") + "_pepper_polished.fastq").read() == "@a\nACG\n+\n+5?\n"      # nothing of contig c


def test_off_changes_nothing(tmp_path):
    pred = tmp_path / "pred"
    write_rows_no_pipeline_would_write(pred)
    fasta, _ = host_texts(pred, tmp_path / "on" / "asm", 3)
    for call in (lambda: perform_stitch(str(pred), str(tmp_path / "off" / "asm"), 3),
                 lambda: perform_stitch(str(pred), str(tmp_path / "off2" / "asm"), 3, qualities=False)):
        out = call()
        assert open(out).read() == fasta
        assert os.listdir(os.path.dirname(out)) == ["asm_pepper_polished.fa"]


def test_signatures_and_switch(monkeypatch):
    from pepper_amd.polish import Stitch
    from pepper_amd.polish.DeviceStitch import DeviceStitcher, stitch_directory
    from pepper_amd.polish.fused import FusedConsensus
    from pepper_amd.polish.polish import polish
    assert inspect.signature(polish).parameters["qualities"].default is None
    for fn in (perform_stitch, Stitch.small_chunk_stitch, Stitch.create_consensus_sequence, stitch_directory, DeviceStitcher.finish):
        assert inspect.signature(fn).parameters["qualities"].default is False, fn
    assert inspect.signature(DeviceStitcher.add).parameters["phred"].default is None
    assert "qualities" in inspect.signature(FusedConsensus.__init__).parameters and hasattr(DeviceStitcher, "write_fastq")
    monkeypatch.delenv("PEPPER_AMD_POLISH_QUALITIES", raising=False)
    assert _lib.polish_qualities() is False
    monkeypatch.setenv("PEPPER_AMD_POLISH_QUALITIES", "1")
    assert _lib.polish_qualities() is True
    monkeypatch.setenv("PEPPER_AMD_POLISH_QUALITIES", "true")
    assert _lib.polish_qualities() is False
    assert _lib.POLISH_QUALITIES_ENV == "PEPPER_AMD_POLISH_QUALITIES"
    assert {"pa_stitcher_add_qual", "pa_stitcher_take_qualities"} <= {name for name, _, _ in _lib.SYMBOLS}


def test_new_symbols_load_and_no_device_is_loud():
    import torch
    from pepper_amd import build
    from pepper_amd.polish.DeviceStitch import DeviceStitcher
    build.build()
    lib = _lib.load()
    assert hasattr(lib, "pa_stitcher_add_qual") and hasattr(lib, "pa_stitcher_take_qualities")
    assert lib.pa_stitcher_take_qualities(None, None, 0) == _lib.PA_ERR_INVALID
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PepperAmdError, match="no CPU fallback"):
            DeviceStitcher(0)
