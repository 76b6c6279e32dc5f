"""polish(..., vcf=True, fill=True) in three forms -- fused with the device stitch, three-step with the device stitch, host
stitch -- writes one and the same .vcf.gz (decompressed bytes), and replaying its records over the draft gives the FASTA of the
run, contig by contig; the same with min_quality and qualities on.  The job is the one of tests/test_gpu_polish_fill_pipeline.py
(a 4 300-base draft, 220 reads, a second contig no read names); batch_invariant=True, so every run has the same labels and phred."""
import glob
import os

import numpy as np
import pytest
import torch

import polish_edits_cases as cases
from pepper_amd import synthetic
from pepper_amd.polish import Variants
from pepper_amd.variant.bgzf import parse_tbi, read_bgzf

pytestmark = pytest.mark.gpu

THREADS = 3
OTHER = "acgtNNacgtTTGGaa" * 12 + "n"
FORMS = {
    "fused_device": dict(fused_inference=True, device_stitch=True),
    "three_step_device": dict(fused_inference=False, device_stitch=True),
    "three_step_host": dict(fused_inference=False, device_stitch=False),
}
OPTIONS = {
    "plain": dict(),
    "gated": dict(qualities=True, edits=True),     # and min_quality = run.q, the median QUAL of the plain run's records
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """run(form, options) -> (output directory, FASTA, decompressed VCF, stage_walls); every run is made once."""
    import bam_utils as bu
    import pileup_utils as pu
    from pepper_amd.polish.polish import polish
    tmp = tmp_path_factory.mktemp("polish_vcf_job")
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

    def run(form, options):
        if (form, options) not in done:
            out_dir = str(tmp / (form + "_" + options)) + "/"
            walls = {}
            extra = dict(OPTIONS[options], min_quality=run.q) if options == "gated" else OPTIONS[options]
            polish(bam_path, fa_path, out_dir, THREADS, None, model_path, 64, True, "0", 0, batch_invariant=True, stage_walls=walls,
                   fill=True, vcf=True, **extra, **FORMS[form])
            found = glob.glob(out_dir + "*.vcf.gz")
            assert len(found) == 1 and found[0].endswith("_pepper_polished.vcf.gz") and os.path.exists(found[0] + ".tbi")
            assert parse_tbi(found[0] + ".tbi")["names"] == ["ctg1"]
            done[(form, options)] = (out_dir, open(glob.glob(out_dir + "*.fa")[0]).read(), read_bgzf(found[0]).decode(), walls)
        return done[(form, options)]
    run.drafts, run.args = {"ctg1": draft, "ctg2": OTHER}, (bam_path, fa_path, model_path, str(tmp))
    # the gate: a QUAL that splits the plain run's records (the median; where that is the lowest there is, the next one above it)
    qual = np.sort([int(line.split("\t")[5]) for line in run("three_step_host", "plain")[2].splitlines() if not line.startswith("#")])
    assert qual.size > 10 and qual[0] < qual[-1]
    run.q = int(np.median(qual)) if qual[0] < int(np.median(qual)) else int(qual[qual > qual[0]][0])
    return run


@pytest.mark.parametrize("options", list(OPTIONS))
@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_writes_the_same_vcf_and_it_replays_to_the_fasta(runs, form, options):
    out_dir, fasta, vcf, walls = runs(form, options)
    assert vcf == runs("three_step_host", options)[2] and fasta == runs("three_step_host", options)[1]
    assert vcf.startswith(Variants.header([(name, len(seq)) for name, seq in runs.drafts.items()]))
    calls = Variants.parse(vcf)
    assert list(calls) == ["ctg1"] and len(calls["ctg1"]) > 10
    sequences = cases.fasta_sequences(fasta)
    for contig, draft in runs.drafts.items():
        assert Variants.replay(draft, calls.get(contig, [])) == sequences[contig].upper()
    body = [line.split("\t") for line in vcf.splitlines() if not line.startswith("#")]
    assert all(f[5].isdigit() and f[6:] == ["PASS", ".", "GT:GQ", "1:" + f[5]] and f[3] != f[4] for f in body)
    if options == "gated":                                          # exactly the applied edits: no record is below the gate
        assert min(int(f[5]) for f in body) >= runs.q and vcf != runs(form, "plain")[2] and fasta != runs(form, "plain")[1]
    if form == "fused_device":
        totals = walls["device_stitch_vcf"]
        assert set(totals) == {"records", "noops", "unanchored", "shifted", "bytes_returned", "seconds_device", "seconds_text"}
        assert totals["records"] == len(body) and totals["bytes_returned"] == 32 * len(body) and totals["unanchored"] == 0
        assert totals["seconds_device"] > 0 and totals["seconds_text"] > 0


def test_vcf_without_fill_raises_before_any_file_is_written(runs, monkeypatch):
    from pepper_amd import _lib
    from pepper_amd.polish.polish import polish
    bam_path, fa_path, model_path, tmp = runs.args
    out_dir = tmp + "/refused/"
    for kw in (dict(vcf=True), dict(vcf=True, fill=False, fused_inference=True, device_stitch=True)):
        with pytest.raises(ValueError, match="vcf needs fill"):
            polish(bam_path, fa_path, out_dir, THREADS, None, model_path, 64, True, "0", 0, **kw)
    monkeypatch.setenv(_lib.POLISH_VCF_ENV, "1")
    with pytest.raises(ValueError, match="vcf needs fill"):
        polish(bam_path, fa_path, out_dir, THREADS, None, model_path, 64, True, "0", 0)
    assert not os.path.exists(out_dir)
