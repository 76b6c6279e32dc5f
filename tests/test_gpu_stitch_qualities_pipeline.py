"""polish(..., qualities=True) in its five forms -- three-step or fused, host or device stitch, the fused device form with and
without prediction files -- writes one and the same FASTQ beside a FASTA that does not change.  The job is the one of
tests/test_gpu_device_stitch_pipeline.py (a 4 300-base draft, 220 reads); batch_invariant=True, so every run has the same labels
and the same phred."""
import glob

import numpy as np
import pytest
import torch

from pepper_amd import synthetic
from pepper_amd.polish.perform_stitch import perform_stitch

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
    """run(form, qualities) -> (output directory, FASTA text, FASTQ text or None); every run is made once."""
    import bam_utils as bu
    import pileup_utils as pu
    from pepper_amd.polish.polish import polish
    tmp = tmp_path_factory.mktemp("stitch_qualities_job")
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

    def run(form, qualities, tag=""):
        key = (form, qualities, tag)
        if key not in done:
            out_dir = str(tmp / ("%s_%s%s" % (form, {True: "on", False: "off", None: "default"}[qualities], tag))) + "/"
            kw = dict(FORMS[form])
            if qualities is not None:
                kw["qualities"] = qualities
            polish(bam_path, fa_path, out_dir, THREADS, None, model_path, 64, True, "0", 0, batch_invariant=True, **kw)
            fasta = glob.glob(out_dir + "*.fa")
            assert len(fasta) == 1 and fasta[0].endswith("_pepper_polished.fa")
            fastq = glob.glob(out_dir + "*.fastq")
            assert len(fastq) <= 1
            done[key] = (out_dir, open(fasta[0]).read(), open(fastq[0]).read() if fastq else None)
        return done[key]
    return run


@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_writes_the_same_fastq(runs, form):
    _, fasta, fastq = runs(form, True)
    _, ref_fasta, ref_fastq = runs("three_step_host", True)
    assert fastq is not None and (fasta, fastq) == (ref_fasta, ref_fastq)
    name, seq, plus, qual = fastq.splitlines()
    assert name == "@ctg1" and plus == "+" and seq == fasta.splitlines()[1] and len(qual) == len(seq) > 2000
    assert len(set(qual)) > 3 and all(33 <= ord(c) <= 126 for c in qual)


@pytest.mark.parametrize("form", list(FORMS))
def test_fasta_is_the_one_with_qualities_off(runs, form):
    out_dir, fasta, fastq = runs(form, False)
    assert fastq is None and not glob.glob(out_dir + "*.fastq")
    assert fasta == runs(form, True)[1]


def test_lean_form_leaves_no_prediction_file(runs):
    out_dir, _, _ = runs("fused_device_lean", True)
    assert glob.glob(out_dir + "predictions_*/") and not glob.glob(out_dir + "predictions_*/*")


def test_kept_form_matches_the_host_stitch_of_its_files(runs, tmp_path):
    out_dir, fasta, fastq = runs("fused_device_kept", True)
    pred = glob.glob(out_dir + "predictions_*/")
    assert len(pred) == 1 and glob.glob(pred[0] + "*.hdf")
    prefix = str(tmp_path / "host") + "/"
    out = perform_stitch(pred[0], prefix, THREADS, qualities=True)
    assert open(out).read() == fasta and open(prefix + "_pepper_polished.fastq").read() == fastq


def test_environment_switch(runs, monkeypatch):
    monkeypatch.setenv("PEPPER_AMD_POLISH_QUALITIES", "1")
    out_dir, fasta, fastq = runs("fused_device_lean", None, "_env")
    assert (fasta, fastq) == runs("three_step_host", True)[1:]
    assert not glob.glob(out_dir + "predictions_*/*")
