"""polish(..., edits=True) in its forms -- three-step or fused, host or device stitch, the fused device form with and without
prediction files -- writes one and the same .edits.tsv beside a FASTA that does not change, and the records replayed over the
draft give that FASTA.  The job is the one of tests/test_gpu_stitch_qualities_pipeline.py (a 4 300-base draft, 220 reads);
batch_invariant=True, so every run has the same labels and the same phred."""
import glob
import io

import numpy as np
import pytest
import torch

import polish_edits_cases as cases
from pepper_amd import synthetic
from pepper_amd.polish import Edits

pytestmark = pytest.mark.gpu

THREADS = 3                                    # five intervals -> pieces of max(2, int(5 / 3) + 1) = 2 regions: three pieces

FORMS = {
    "three_step_host": dict(fused_inference=False, device_stitch=False),
    "three_step_device": dict(fused_inference=False, device_stitch=True),
    "fused_host": dict(fused_inference=True, device_stitch=False),
    "fused_device_kept": dict(fused_inference=True, device_stitch=True, keep_predictions=True),
    "fused_device_lean": dict(fused_inference=True, device_stitch=True),
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """run(form, edits) -> (output directory, FASTA text, .edits.tsv text or None); every run is made once.  run.draft: the
    draft, run.fa_path: its FASTA."""
    import bam_utils as bu
    import pileup_utils as pu
    from pepper_amd.polish.polish import polish
    tmp = tmp_path_factory.mktemp("polish_edits_job")
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

    def run(form, edits, tag=""):
        key = (form, edits, tag)
        if key not in done:
            out_dir = str(tmp / ("%s_%s%s" % (form, {True: "on", False: "off", None: "default"}[edits], tag))) + "/"
            kw = dict(FORMS[form])
            if edits is not None:
                kw["edits"] = edits
            polish(bam_path, fa_path, out_dir, THREADS, None, model_path, 64, True, "0", 0, batch_invariant=True, **kw)
            fasta = glob.glob(out_dir + "*.fa")
            assert len(fasta) == 1 and fasta[0].endswith("_pepper_polished.fa")
            tsv = glob.glob(out_dir + "*.edits.tsv")
            assert len(tsv) <= 1 and not glob.glob(out_dir + "*.fastq")
            done[key] = (out_dir, open(fasta[0]).read(), open(tsv[0]).read() if tsv else None)
        return done[key]
    run.draft, run.fa_path = draft, fa_path
    return run


@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_writes_the_same_edits(runs, form):
    _, fasta, tsv = runs(form, True)
    _, ref_fasta, ref_tsv = runs("three_step_host", True)
    assert tsv is not None and (fasta, tsv) == (ref_fasta, ref_tsv)
    lines = tsv.splitlines()
    assert lines[0] + "\n" == Edits.HEADER and lines[-1].startswith("##contig=ctg1\tdraft_length=4300\tpolished_length=%d\t" %
                                                                   len(fasta.splitlines()[1]))
    assert len(lines) > 20 and all(line.split("\t")[0] == "ctg1" and len(line.split("\t")) == 9 for line in lines[1:-1])
    assert any(line.split("\t")[-1].isdigit() for line in lines[1:-1])          # the phred reached the stitcher in every form


@pytest.mark.parametrize("form", list(FORMS))
def test_fasta_is_the_one_with_edits_off(runs, form):
    out_dir, fasta, tsv = runs(form, False)
    assert tsv is None and not glob.glob(out_dir + "*.tsv")
    assert fasta == runs(form, True)[1]


def test_lean_form_leaves_no_prediction_file(runs):
    out_dir, _, _ = runs("fused_device_lean", True)
    assert glob.glob(out_dir + "predictions_*/") and not glob.glob(out_dir + "predictions_*/*")


def test_apply_over_the_draft_reproduces_the_fasta(runs):
    """The records of the kept form's prediction files (the numpy twin), replayed over the draft."""
    out_dir, fasta, tsv = runs("fused_device_kept", True)
    pred = glob.glob(out_dir + "predictions_*/")
    assert len(pred) == 1 and glob.glob(pred[0] + "*.hdf")
    sequence, records, pieces = cases.host_records(pred[0], runs.fa_path, "ctg1", THREADS)
    assert len(pieces) == 3 and len(records) > 20
    assert Edits.apply(runs.draft, records, pieces) == sequence == fasta.splitlines()[1]
    text = io.StringIO()
    text.write(Edits.HEADER)
    Edits.write_contig(text, "ctg1", records, pieces, len(runs.draft), True)
    assert text.getvalue() == tsv


def test_environment_switch(runs, monkeypatch):
    monkeypatch.setenv("PEPPER_AMD_POLISH_EDITS", "1")
    out_dir, fasta, tsv = runs("fused_device_lean", None, "_env")
    assert (fasta, tsv) == runs("three_step_host", True)[1:]
    assert not glob.glob(out_dir + "predictions_*/*")
