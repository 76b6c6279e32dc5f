"""polish(..., min_quality=Q, qualities=True, edits=True) in its four forms -- three-step or fused, host or device stitch -- writes one
and the same gated consensus: FASTA, FASTQ, .edits.tsv and .withheld.tsv byte for byte.  The job is the one of
tests/test_gpu_polish_fill_pipeline.py (a 4 300-base draft, 220 reads); batch_invariant=True, so every run has the same labels and
the same phred.  Q is the median phred of the SUB / DEL / INS records of an ungated run, so that some edits are applied and some
withheld."""
import glob

import numpy as np
import pytest
import torch

import polish_edits_cases as cases
from pepper_amd import synthetic
from pepper_amd.polish import Edits
from pepper_amd.polish.Stitch import create_consensus_sequence

pytestmark = pytest.mark.gpu

THREADS = 3                                    # five intervals: three pieces
PATTERNS = ("*.fa", "*.fastq", "*.edits.tsv", "*.withheld.tsv")

FORMS = {
    "three_step_host": dict(fused_inference=False, device_stitch=False),
    "three_step_device": dict(fused_inference=False, device_stitch=True),
    "fused_host": dict(fused_inference=True, device_stitch=False),
    "fused_device": dict(fused_inference=True, device_stitch=True),
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """run(form, min_quality) -> (output directory, FASTA, FASTQ, .edits.tsv, .withheld.tsv or None, stage_walls); every run is
    made once.  run.q: the gate, from the ungated three-step host run."""
    import bam_utils as bu
    import pileup_utils as pu
    from pepper_amd.polish.polish import polish
    tmp = tmp_path_factory.mktemp("polish_gate_job")
    rng = np.random.default_rng(91)
    draft = pu.random_reference(rng, 4300)
    reads = pu.simulate_reads(rng, draft, 0, n_reads=220, read_len=(600, 2500), ins_rate=0.02, del_rate=0.02)
    reads = [r for r in reads if not any(op in (3, 6) for op, _ in r["cigar"])]
    for i, r in enumerate(reads):
        r["name"] = "q%d" % i
    bam_path, fa_path = str(tmp / "reads.bam"), str(tmp / "draft.fa")
    bu.write_bam(bam_path, [("ctg1", len(draft))], {0: reads})
    with open(fa_path, "w") as fh:
        fh.write(">ctg1\n" + draft + "\n")
    sd = synthetic.polish_state_dict(seed=17, gain=2.0)
    model_path = str(tmp / "polish.pkl")
    torch.save(synthetic.checkpoint_dict({k: torch.from_numpy(v) for k, v in sd.items()}, hidden_size=128), model_path)
    done = {}

    def run(form, min_quality, tag=""):
        if (form, min_quality, tag) not in done:
            out_dir = str(tmp / ("%s_%s%s" % (form, min_quality, tag))) + "/"
            walls = {}
            polish(bam_path, fa_path, out_dir, THREADS, None, model_path, 64, True, "0", 0, batch_invariant=True, stage_walls=walls,
                   qualities=True, edits=True, min_quality=min_quality, **FORMS[form])
            texts = []
            for pattern in PATTERNS:
                found = glob.glob(out_dir + pattern)
                assert len(found) <= 1
                texts.append(open(found[0]).read() if found else None)
            done[(form, min_quality, tag)] = (out_dir,) + tuple(texts) + (walls,)
        return done[(form, min_quality, tag)]

    # the gate: the median phred of what the ungated consensus changed
    out_dir = run("three_step_host", 0)[0]
    pred = glob.glob(out_dir + "predictions_*/")
    assert len(pred) == 1
    _, _, records, _ = create_consensus_sequence("ctg1", cases.contig_keys(pred[0], "ctg1"), THREADS, qualities=True, edits=fa_path)
    assert set(draft) <= set("ACGT")             # (every SUB and DEL stands on a base: the gate may withhold any of them)
    phred = np.sort(records["phred"][records["kind"] < Edits.GAP_OPEN].astype(np.int64))
    assert phred.size > 20 and phred[0] < phred[-1]
    q = int(np.median(phred))
    if not phred[0] < q:                       # (the median is the lowest phred there is: the next value above it splits the set)
        q = int(phred[phred > phred[0]][0])
    run.q, run.ungated_phred, run.draft, run.fa_path = q, phred, draft, fa_path
    return run


@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_writes_the_same_gated_files(runs, form):
    q = runs.q
    assert 1 <= q <= 255
    out_dir, fasta, fastq, tsv, withheld, walls = runs(form, q)
    want = runs("three_step_host", q)
    assert (fasta, fastq, tsv, withheld) == want[1:5] and all(text for text in want[1:5])
    ungated = runs("three_step_host", 0)
    assert ungated[4] is None and "withheld=" not in ungated[3] and fasta != ungated[1]
    # both sets are there: the withheld edits lie below the gate, what is left of the ungated edits at or above it
    held = [line.split("\t") for line in withheld.splitlines()[1:]]
    assert len(held) == int((runs.ungated_phred < q).sum()) > 0 and all(int(line[6]) < q for line in held)
    assert int((runs.ungated_phred >= q).sum()) > 0
    summary = [line for line in tsv.splitlines() if line.startswith("##contig=ctg1\t")]
    assert len(summary) == 1 and summary[0].split("\t")[-1] == "withheld=%d" % len(held)
    hunks = [line for line in tsv.splitlines()[1:] if not line.startswith("##") and line.split("\t")[5] in ("sub", "ins", "del", "complex")]
    assert len(hunks) > 0 and all(line.split("\t")[8] == "." or int(line.split("\t")[8]) >= q for line in hunks)
    sequence = cases.fasta_sequences(fasta)["ctg1"]
    lines = fastq.splitlines()
    assert lines[1] == sequence and len(lines[3]) == len(sequence)
    for line in held:                                                # a kept letter stands in the consensus with quality '!'
        if line[3] != "ins":
            assert sequence[int(line[7])] == line[4] == runs.draft[int(line[1])].upper() and lines[3][int(line[7])] == "!"
    if form == "fused_device":
        assert not glob.glob(out_dir + "predictions_*/*")            # still no prediction file
        gate = walls["device_stitch_gate"]
        assert set(gate) == {"withheld", "sub", "del", "ins", "bytes_returned", "seconds"}
        assert gate["withheld"] == len(held) == gate["sub"] + gate["del"] + gate["ins"] and gate["bytes_returned"] == 16 * len(held)
        assert gate["seconds"] > 0
    else:
        assert "device_stitch_gate" not in walls


def test_the_applied_records_replay_to_the_fasta(runs):
    """The records of the three-step form's prediction files (the host form) under the gate, replayed over the draft."""
    out_dir, fasta, fastq, tsv, withheld, _ = runs("three_step_device", runs.q)
    pred = glob.glob(out_dir + "predictions_*/")
    assert len(pred) == 1 and glob.glob(pred[0] + "*.hdf")
    sequence, quality, records, pieces, held = create_consensus_sequence("ctg1", cases.contig_keys(pred[0], "ctg1"), THREADS,
                                                                         qualities=True, edits=runs.fa_path, min_quality=runs.q,
                                                                         draft=runs.fa_path)
    assert len(pieces) == 3 and len(records) > 20 and len(held) == len(withheld.splitlines()) - 1
    assert Edits.apply(runs.draft, records, pieces) == sequence == cases.fasta_sequences(fasta)["ctg1"]
    assert quality == fastq.splitlines()[3]


def test_environment_switch(runs, monkeypatch):
    """PEPPER_AMD_POLISH_MIN_QUALITY=Q is min_quality=Q."""
    from pepper_amd import _lib
    monkeypatch.setenv("PEPPER_AMD_POLISH_MIN_QUALITY", str(runs.q))
    assert _lib.polish_min_quality() == runs.q
    assert runs("fused_device", None, "_env")[1:5] == runs("three_step_host", runs.q)[1:5]
    monkeypatch.setenv("PEPPER_AMD_POLISH_MIN_QUALITY", "0")
    assert _lib.polish_min_quality() is None
    monkeypatch.setenv("PEPPER_AMD_POLISH_MIN_QUALITY", "300")
    with pytest.raises(ValueError):
        _lib.polish_min_quality()
