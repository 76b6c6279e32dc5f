"""FastCandidates.process_segments -- the candidate finder of a run that has no prediction file (the fused call_variant with
device_selection) -- against process() from the prediction files of the same batches, and the switch's default and parsing."""
import os
import random

import numpy as np

from pepper_amd import _lib
from pepper_amd.variant import FastCandidates, bgzf
from pepper_amd.variant.DataStorePredict import DataStore
from pepper_amd.variant.FindCandidates import process_candidates
from test_candidate_finder import _resolved, options


def _calls(tmp_path, n, seed):
    """Prediction batches shaped like encoder calls: one contig each, ascending positions, a site's rows (up to three allele
    records, some of them the same (REF, ALT) twice) all in ONE batch; low-complexity stretches, N bases, alleles outside ACGT."""
    rng = np.random.default_rng(seed)
    length = 12 * n + 1000
    pieces = []
    while sum(len(p) for p in pieces) < length:
        pieces.append("ACGTN"[int(rng.choice(5, p=[0.24, 0.24, 0.24, 0.24, 0.04]))] * int(rng.choice([1, 1, 1, 1, 2, 3, 6, 8])))
    refs = {"chrB": "".join(pieces)[:length], "chrA": "".join(reversed(pieces))[:length]}
    fa = str(tmp_path / "syn.fa")
    with open(fa, "w") as fh:
        for name, seq in refs.items():
            fh.write(">" + name + "\n" + "\n".join(seq[i:i + 70] for i in range(0, length, 70)) + "\n")
    pred_dir = tmp_path / "pred"
    pred_dir.mkdir()
    multi = 0
    for fi, contig in enumerate(("chrB", "chrA")):
        ref = refs[contig]
        store = DataStore(str(pred_dir / ("pepper_prediction_%d.hdf" % fi)), "w")
        sites = np.sort(rng.choice(np.arange(50, length - 50), n // 2, replace=False))
        copies = rng.choice([1, 1, 1, 1, 1, 1, 1, 2, 3], len(sites))
        multi += int((copies > 1).sum())
        batch, at = 0, 0
        while at < len(sites):
            take = int(rng.integers(40, 200))                                  # sites of this call
            pos = np.repeat(sites[at:at + take], copies[at:at + take]).astype(np.int32)
            at += take
            m = len(pos)
            cands = []
            for p in pos:
                r = ref[int(p)] if ref[int(p)] in "ACGT" else "A"
                k = int(rng.integers(0, 6))
                if k <= 1:
                    cands.append(["1" + "ACGT"[("ACGT".index(r) + 1 + k) % 4]])
                elif k == 2:
                    cands.append(["2" + r + "ACGTT"[: int(rng.integers(1, 5))]])
                elif k == 3:
                    cands.append(["3" + ref[int(p):int(p) + int(rng.integers(2, 6))].replace("N", "A")])
                elif k == 4:
                    cands.append(["1N"])
                else:
                    cands.append(["2" + r + "A"])
            probs = rng.dirichlet([0.6, 0.6, 0.6], m)
            store.write_prediction(batch, [contig] * m, pos, rng.integers(1, 90, m).astype(np.uint8), np.array(cands, dtype=object),
                                   rng.integers(0, 60, (m, 1)).astype(np.uint8), probs)
            batch += 1
        store.close()
    assert multi > 0
    return fa, str(pred_dir)


def test_process_segments_writes_the_files_of_process(tmp_path):
    fa, pred_dir = _calls(tmp_path, 1500, 9)
    opts = options(fasta=fa, report_snp_above_freq=0.2, report_indel_above_freq=0.2, allowed_multiallelics=2)
    want_totals = process_candidates(opts, pred_dir, str(tmp_path / "files"))
    assert want_totals[0] > 300 and want_totals[1] > 0 and want_totals[3] > 0 and want_totals[4] > 0
    # the same batches as segments, each through native_batch_arrays (what _native_batch reads a file's batch for)
    from pepper_amd import h5
    from pepper_amd.variant.FindCandidates import get_file_paths_from_directory
    rules = FastCandidates._rules(opts)
    fasta_handler = FastCandidates._fasta(opts)
    segments = []
    for name in get_file_paths_from_directory(pred_dir):
        with h5.File(name, "r") as f:
            keys = list(f.keys("predictions"))
        for key in keys:
            seg = FastCandidates._native_batch(opts, rules, fasta_handler, name, key)
            assert seg is not None
            segments.append(seg)
    assert len(segments) > 10 and all(len(seg) > 0 for seg in segments)
    multi = sum(int((np.diff(seg.pos) == 0).sum()) for seg in segments)
    assert multi > 20                                                          # sites with several allele records
    for tag, order in (("listed", list(segments)), ("shuffled", random.Random(4).sample(segments, len(segments))),
                       ("reversed", segments[::-1])):
        out = str(tmp_path / tag)
        got_totals = process_candidates(opts, None, out, segments=order)
        assert tuple(got_totals) == tuple(want_totals), tag
        names = sorted(os.listdir(tmp_path / "files"))
        assert names == sorted(os.listdir(out)) and len([x for x in names if x.endswith(".vcf.gz")]) == 5
        for name in names:
            a, b = str(tmp_path / "files" / name), os.path.join(out, name)
            if name.endswith(".tbi"):
                assert _resolved(bgzf.parse_tbi(a), a[:-4]) == _resolved(bgzf.parse_tbi(b), b[:-4]), (tag, name)
            else:
                assert bgzf.read_bgzf(a) == bgzf.read_bgzf(b), (tag, name)


def test_process_segments_without_rows(tmp_path):
    fa, _ = _calls(tmp_path, 200, 3)
    opts = options(fasta=fa)
    empty = FastCandidates._Segment("chrA", np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, bool), np.zeros(0, bool), [])
    assert tuple(process_candidates(opts, None, str(tmp_path / "none"), segments=[])) == (0, 0, 0, 0, 0)
    assert tuple(process_candidates(opts, None, str(tmp_path / "empty"), segments=[empty])) == (0, 0, 0, 0, 0)


def test_device_selection_switch(monkeypatch):
    """Off unless PEPPER_AMD_DEVICE_SELECTION is exactly 1, as device_stitch reads its variable."""
    assert _lib.DEVICE_SELECTION_ENV == "PEPPER_AMD_DEVICE_SELECTION"
    monkeypatch.delenv(_lib.DEVICE_SELECTION_ENV, raising=False)
    assert _lib.device_selection() is False
    for value, want in (("1", True), ("0", False), ("", False), ("true", False), ("2", False)):
        monkeypatch.setenv(_lib.DEVICE_SELECTION_ENV, value)
        assert _lib.device_selection() is want, value


def test_select_host_takes_the_python_path_for_a_call_the_library_refuses(tmp_path):
    """FusedPredictor.select_host (the lean fused run's way for host-clipped groups and handed-back calls): a call with a NaN
    probability, which pa_candidates_select_format refuses, gives the records the candidate finder gives from a prediction file
    of the same rows; the file it borrows for the per-row path is withdrawn again."""
    from pepper_amd.variant.fused import FusedPredictor
    rng = np.random.default_rng(12)
    fa, _ = _calls(tmp_path, 200, 3)
    contig = "chrA"
    n = 60
    pos = np.sort(rng.choice(np.arange(100, 2000), n, replace=False)).astype(np.int32)
    cands = [["1" + "ACGT"[int(k)]] for k in rng.integers(0, 4, n)]
    depths, freqs = rng.integers(1, 90, n).astype(np.uint8), rng.integers(0, 60, (n, 1)).astype(np.uint8)
    probs = rng.dirichlet([0.6, 0.6, 0.6], n).astype(np.float32)
    probs[7, 1] = np.nan
    pred_dir = tmp_path / "nan_pred"
    pred_dir.mkdir()
    store = DataStore(str(pred_dir / "pepper_prediction.hdf"), "w")
    store.write_prediction(0, [contig] * n, pos, depths, np.array(cands, dtype=object), freqs, probs)
    store.close()
    opts = options(fasta=fa, device_selection=True, batch_size=128)
    want_totals = process_candidates(opts, str(pred_dir), str(tmp_path / "from_file"))
    assert want_totals[0] > 10
    lean_dir = tmp_path / "lean_pred"
    lean_dir.mkdir()
    sink = FusedPredictor(opts, str(lean_dir) + "/")
    assert sink.writer is None and sink.selector is None and sink.store is None
    out = dict(positions=pos.astype(np.int64), depths=depths.astype(np.int32), candidate_frequency=freqs[:, 0].astype(np.int32),
               candidates=[c[0] for c in cands])
    half = n // 2
    cut = lambda d, a, b: {k: v[a:b] for k, v in d.items()}      # noqa: E731 -- two intervals of one call
    sink.select_host(contig, [cut(out, 0, half), cut(out, half, n)], probs)
    sink.close()
    assert os.listdir(lean_dir) == [] and len(sink.device_segments) == 1
    got_totals = process_candidates(opts, None, str(tmp_path / "from_segments"), segments=sink.device_segments)
    assert tuple(got_totals) == tuple(want_totals)
    for name in sorted(os.listdir(tmp_path / "from_file")):
        if name.endswith(".vcf.gz"):
            assert bgzf.read_bgzf(str(tmp_path / "from_file" / name)) == bgzf.read_bgzf(str(tmp_path / "from_segments" / name)), name
