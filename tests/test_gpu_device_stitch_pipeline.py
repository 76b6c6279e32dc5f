"""polish(..., device_stitch=True): the FASTA of the fused and of the three-step run is the one perform_stitch writes from the
same predictions with the same `threads`; the fused run writes prediction files only when asked to; with the switch off nothing
changes.  The job is the one of test_polish_end_to_end_from_bam (a 4 300-base draft, 220 reads); batch_invariant=True, so every
run has the same labels."""
import glob
import os

import numpy as np
import pytest
import torch

from pepper_amd import synthetic
from pepper_amd.polish.perform_stitch import perform_stitch

pytestmark = pytest.mark.gpu

THREADS = 3                                    # five intervals -> pieces of max(2, int(5 / 3) + 1) = 2 regions: three pieces


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    import bam_utils as bu
    import pileup_utils as pu
    from pepper_amd.polish.polish import polish
    tmp = tmp_path_factory.mktemp("device_stitch_job")
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

    def run(name, **kw):
        out_dir = str(tmp / name) + "/"
        walls = {}
        polish(bam_path, fa_path, out_dir, THREADS, None, model_path, 64, True, "0", 0, stage_walls=walls, batch_invariant=True, **kw)
        fasta = glob.glob(out_dir + "*.fa")
        assert len(fasta) == 1 and fasta[0].endswith("_pepper_polished.fa")
        return out_dir, open(fasta[0]).read(), walls
    return run, len(draft)


@pytest.fixture(scope="module")
def host_fused(job, tmp_path_factory):
    """The fused run with the switch off: (FASTA text, its prediction files)."""
    run, _ = job
    os.environ.pop("PEPPER_AMD_DEVICE_STITCH", None)
    out_dir, text, walls = run("fused_host", fused_inference=True)
    return out_dir, text, walls


def _host_stitch(out_dir, where):
    pred = glob.glob(out_dir + "predictions_*/")
    assert len(pred) == 1
    return open(perform_stitch(pred[0], str(where) + "/", THREADS)).read()


def test_switch_off_changes_nothing(job, host_fused, tmp_path):
    _, draft_len = job
    out_dir, text, walls = host_fused
    assert "device_stitch_stats" not in walls
    files = sorted(os.path.basename(p) for p in glob.glob(out_dir + "predictions_*/*.hdf"))
    assert files and all(f.startswith("pepper_prediction_fused_") for f in files)
    assert glob.glob(out_dir + "images_*/*.hdf")
    assert text == _host_stitch(out_dir, tmp_path / "again")
    assert text.startswith(">ctg1\n") and 0.5 * draft_len < len(text.split("\n", 1)[1].strip()) < 2 * draft_len


def test_fused_with_predictions_kept(job, host_fused, tmp_path):
    run, _ = job
    out_dir, text, walls = run("fused_keep", fused_inference=True, device_stitch=True, keep_predictions=True)
    assert glob.glob(out_dir + "predictions_*/*.hdf")
    assert text == _host_stitch(out_dir, tmp_path / "host")          # the predictions THAT run left, the same threads
    assert text == host_fused[1]
    stats = walls["device_stitch_stats"]
    assert stats["pieces"] == 3 and stats["rows"] > 4000 and stats["slots"] >= stats["positions"] > 4000


def test_fused_without_prediction_files(job, host_fused):
    run, _ = job
    out_dir, text, walls = run("fused_lean", fused_inference=True, device_stitch=True)
    assert text == host_fused[1]
    assert glob.glob(out_dir + "predictions_*/") and not glob.glob(out_dir + "predictions_*/*")
    assert walls["call_consensus"] == 0 and walls["perform_stitch"] > 0


def test_three_step_with_device_stitch(job, host_fused, tmp_path):
    run, _ = job
    out_dir, text, _ = run("three_step", fused_inference=False, device_stitch=True)
    assert text == _host_stitch(out_dir, tmp_path / "host")
    assert text == host_fused[1]


def test_environment_switch(job, host_fused, monkeypatch):
    run, _ = job
    monkeypatch.setenv("PEPPER_AMD_DEVICE_STITCH", "1")
    out_dir, text, walls = run("fused_env", fused_inference=True)
    assert text == host_fused[1] and "device_stitch_stats" in walls and not glob.glob(out_dir + "predictions_*/*")
