"""polish(..., fill=True, qualities=True, edits=True) in its four forms -- three-step or fused, host or device stitch -- writes one
and the same complete consensus: FASTA, FASTQ and .edits.tsv byte for byte, every contig of the draft in them.  The job is the one
of tests/test_gpu_polish_edits_pipeline.py (a 4 300-base draft, 220 reads) with a second contig in the draft that no read names;
batch_invariant=True, so every run has the same labels and the same phred."""
import glob

import numpy as np
import pytest
import torch

import polish_edits_cases as cases
from pepper_amd import synthetic
from pepper_amd.polish import Edits
from pepper_amd.polish.Stitch import create_consensus_sequence

pytestmark = pytest.mark.gpu

THREADS = 3                                    # five intervals: three pieces without fill, one with it
OTHER = "acgtNNacgtTTGGaa" * 12 + "n"

FORMS = {
    "three_step_host": dict(fused_inference=False, device_stitch=False),
    "three_step_device": dict(fused_inference=False, device_stitch=True),
    "fused_host": dict(fused_inference=True, device_stitch=False),
    "fused_device": dict(fused_inference=True, device_stitch=True),
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """run(form) -> (output directory, FASTA, FASTQ, .edits.tsv, stage_walls); every run is made once."""
    import bam_utils as bu
    import pileup_utils as pu
    from pepper_amd.polish.polish import polish
    tmp = tmp_path_factory.mktemp("polish_fill_job")
    rng = np.random.default_rng(91)
    draft = pu.random_reference(rng, 4300)
    reads = pu.simulate_reads(rng, draft, 0, n_reads=220, read_len=(600, 2500), ins_rate=0.02, del_rate=0.02)
    reads = [r for r in reads if not any(op in (3, 6) for op, _ in r["cigar"])]
    for i, r in enumerate(reads):
        r["name"] = "q%d" % i
    bam_path, fa_path = str(tmp / "reads.bam"), str(tmp / "draft.fa")
    bu.write_bam(bam_path, [("ctg1", len(draft))], {0: reads})
    with open(fa_path, "w") as fh:
        fh.write(">ctg1\n" + draft + "\n>ctg2\n" + OTHER + "\n")
    sd = synthetic.polish_state_dict(seed=17, gain=2.0)
    model_path = str(tmp / "polish.pkl")
    torch.save(synthetic.checkpoint_dict({k: torch.from_numpy(v) for k, v in sd.items()}, hidden_size=128), model_path)
    done = {}

    def run(form, region=None, fill=True):
        if (form, region, fill) not in done:
            out_dir = str(tmp / (form + ("_region" if region else "") + ("" if fill else "_env"))) + "/"
            walls = {}
            polish(bam_path, fa_path, out_dir, THREADS, region, model_path, 64, True, "0", 0, batch_invariant=True, stage_walls=walls,
                   fill=fill, qualities=True, edits=True, **FORMS[form])
            texts = []
            for pattern in ("*.fa", "*.fastq", "*.edits.tsv"):
                found = glob.glob(out_dir + pattern)
                assert len(found) == 1
                texts.append(open(found[0]).read())
            done[(form, region, fill)] = (out_dir,) + tuple(texts) + (walls,)
        return done[(form, region, fill)]
    run.drafts, run.fa_path = {"ctg1": draft, "ctg2": OTHER}, fa_path
    return run


@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_writes_the_same_complete_consensus(runs, form):
    out_dir, fasta, fastq, tsv, walls = runs(form)
    assert (fasta, fastq, tsv) == runs("three_step_host")[1:4]
    sequences = cases.fasta_sequences(fasta)
    assert list(sequences) == ["ctg1", "ctg2"] and sequences["ctg2"] == OTHER              # every contig of the draft
    lines = fastq.splitlines()
    assert lines[0::4] == ["@ctg1", "@ctg2"] and lines[1::4] == [sequences["ctg1"], sequences["ctg2"]] and lines[7] == "!" * len(OTHER)
    assert any(c != "!" for c in lines[3])
    for contig, draft in runs.drafts.items():                                              # (d) the length adds up
        summary = [line for line in tsv.splitlines() if line.startswith("##contig=" + contig + "\t")]
        assert len(summary) == 1
        s = dict(c.split("=") for c in summary[0].split("\t")[1:])
        assert list(s)[-1] == "filled" and int(s["uncovered"]) == int(s["duplicated"]) == 0
        assert int(s["draft_length"]) == len(draft) and int(s["polished_length"]) == len(sequences[contig]) == \
            len(draft) - int(s["del"]) - int(s["complex_draft"]) + int(s["ins"]) + int(s["complex_polished"])
    assert "\tuncovered\t" not in tsv and "\tduplicated\t" not in tsv and len(tsv.splitlines()) > 20
    if form == "fused_device":
        assert not glob.glob(out_dir + "predictions_*/*")                                  # still no prediction file
        assert set(walls["device_stitch_fill"]) == {"runs", "letters", "seconds"}
        filled = sum(int(line.split("\t")[2]) - int(line.split("\t")[1]) for line in tsv.splitlines() if line.startswith("ctg1\t") and
                     line.split("\t")[5] == "filled")
        assert walls["device_stitch_fill"]["letters"] == filled


def test_apply_over_the_draft_reproduces_the_fasta(runs):
    """(c) the records of the three-step form's prediction files (the host form), replayed over the draft."""
    out_dir, fasta, fastq, tsv, _ = runs("three_step_device")
    pred = glob.glob(out_dir + "predictions_*/")
    assert len(pred) == 1 and glob.glob(pred[0] + "*.hdf")
    sequence, quality, records, pieces = create_consensus_sequence("ctg1", cases.contig_keys(pred[0], "ctg1"), THREADS, qualities=True,
                                                                   edits=runs.fa_path, fill=runs.fa_path)
    assert len(pieces) == 1 and pieces[0][2] == len(sequence) and len(records) > 20
    assert Edits.apply_filled(runs.drafts["ctg1"], records, pieces) == sequence == cases.fasta_sequences(fasta)["ctg1"]
    assert quality == fastq.splitlines()[3]
    assert Edits.apply_filled(runs.drafts["ctg2"], np.zeros(0, Edits.EDIT_DTYPE), []) == OTHER


def test_environment_switch_and_a_region(runs, monkeypatch):
    """PEPPER_AMD_POLISH_FILL=1 is fill=True; with a region only the contigs it names are written."""
    from pepper_amd import _lib
    monkeypatch.setenv("PEPPER_AMD_POLISH_FILL", "1")
    assert _lib.polish_fill() is True
    _, fasta, fastq, tsv, _ = runs("fused_device", "ctg1", None)
    want = runs("three_step_host")
    assert fasta == want[1][:want[1].index(">ctg2")] and fastq == want[2][:want[2].index("@ctg2")]
    assert tsv == ''.join(line + "\n" for line in want[3].splitlines() if "ctg2" not in line)
