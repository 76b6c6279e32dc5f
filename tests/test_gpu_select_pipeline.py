"""The fused call_variant with the candidate finder's selection on the device (options.device_selection /
PEPPER_AMD_DEVICE_SELECTION=1) against the same run with the switch off: the five VCFs line for line, the kept files dataset by
dataset, the lean form without files, every encoder call selected on the device."""
import os

import numpy as np
import pytest

from pepper_amd import h5
from test_gpu_device_candidates_pipeline import job  # noqa: F401 -- the 40 kb job (a module-scoped fixture)
from test_gpu_device_sampling import VCFS, _same_groups, _variant_groups, _variant_options

pytestmark = pytest.mark.gpu

COUNTS = ("encoder_calls", "device_selected_calls", "host_selected_calls", "host_form_intervals")


def _run(job, out, monkeypatch, env=None, freq=0, **over):  # noqa: F811
    from pepper_amd.variant import bgzf
    from pepper_amd.variant.CallVariant import call_variant
    monkeypatch.setenv("PEPPER_AMD_BATCH_INVARIANT", "1")
    monkeypatch.setenv("PEPPER_AMD_DEVICE_CANDIDATES", "1")
    if env is None:
        monkeypatch.delenv("PEPPER_AMD_DEVICE_SELECTION", raising=False)
    else:
        monkeypatch.setenv("PEPPER_AMD_DEVICE_SELECTION", env)
    stats = {}
    o = _variant_options(
        job.bam, job.fasta, None, region=None, region_size=4000, threads=3, output_dir=out, fused_inference=True,
        model_path=job.model, batch_size=128, num_workers=0, gpu=True, device_ids="0", callers_per_gpu=1,
        quantized=False, dry=False, sample_name="SYN", allowed_multiallelics=4,
        snp_p_value=0.1, insert_p_value=0.25, delete_p_value=0.25, snp_p_value_in_lc=0.1,
        insert_p_value_in_lc=0.3, delete_p_value_in_lc=0.3, snp_q_cutoff=20, indel_q_cutoff=15,
        snp_q_cutoff_in_lc=20, indel_q_cutoff_in_lc=10, report_snp_above_freq=freq, report_indel_above_freq=freq,
        stage_seconds=stats)
    del o.image_output_directory
    for k, v in over.items():
        setattr(o, k, v)
    images, predictions, totals = call_variant(o)
    vcfs = {name: bgzf.read_bgzf(os.path.join(out, name + ".vcf.gz")).decode().splitlines() for name in VCFS}
    return dict(images=images, predictions=predictions, totals=tuple(totals), stats=stats, vcfs=vcfs)


def _same_vcfs(got, want):
    assert got["totals"] == want["totals"]
    for name in VCFS:
        assert len(got["vcfs"][name]) == len(want["vcfs"][name]), name
        for g, w in zip(got["vcfs"][name], want["vcfs"][name]):
            assert g == w, (name, g, w)


def _prediction_rows(directory):
    """Every row of a run's prediction files as a sorted list (which batch a row lands in depends on the order the workers'
    intervals arrive in)."""
    rows = []
    for fn in sorted(os.listdir(directory)):
        with h5.File(os.path.join(directory, fn)) as f:
            for key in f.keys("predictions"):
                g = "predictions/" + key + "/"
                contigs, positions, depths = f[g + "contigs"].tolist(), f[g + "positions"], f[g + "depths"]
                cands, freq, pred = f[g + "candidates"].tolist(), f[g + "candidate_frequency"], np.asarray(f[g + "base_prediction"])
                assert pred.dtype == np.float64
                for i in range(len(positions)):
                    rows.append((contigs[i], int(positions[i]), str(cands[i]), int(depths[i]), int(np.ravel(freq[i])[0]), pred[i].tobytes()))
    return sorted(rows)


@pytest.fixture(scope="module")
def switch_off(job, tmp_path_factory):  # noqa: F811
    mp = pytest.MonkeyPatch()
    try:
        return _run(job, str(tmp_path_factory.mktemp("select_off")), mp)
    finally:
        mp.undo()


def test_kept_files_and_vcfs_equal_the_switch_off_run(job, switch_off, tmp_path, monkeypatch):  # noqa: F811
    kept = _run(job, str(tmp_path / "kept"), monkeypatch, device_selection=True, keep_images=True, keep_predictions=True)
    print({k: kept["stats"].get(k) for k in COUNTS})
    assert switch_off["totals"][0] > 30 and switch_off["totals"][2] > 0
    _same_vcfs(kept, switch_off)
    assert _same_groups(_variant_groups(kept["images"]), _variant_groups(switch_off["images"])) > 150
    assert os.listdir(kept["predictions"]) == os.listdir(switch_off["predictions"]) == ["pepper_prediction.hdf"]
    rows = _prediction_rows(kept["predictions"])
    assert rows == _prediction_rows(switch_off["predictions"]) and len(rows) > 150
    assert kept["stats"]["device_selected_calls"] == kept["stats"]["encoder_calls"] and kept["stats"]["host_selected_calls"] == 0
    assert "device_selected_calls" in switch_off["stats"] and switch_off["stats"]["device_selected_calls"] == 0


@pytest.mark.parametrize("through", ["option", "environment"])
def test_lean_run(job, switch_off, tmp_path, monkeypatch, through):  # noqa: F811
    if through == "option":
        lean = _run(job, str(tmp_path / "lean"), monkeypatch, device_selection=True)
    else:
        lean = _run(job, str(tmp_path / "lean"), monkeypatch, env="1")
    print({k: lean["stats"].get(k) for k in COUNTS})
    _same_vcfs(lean, switch_off)
    assert os.path.isdir(lean["images"]) and os.listdir(lean["images"]) == []
    assert os.path.isdir(lean["predictions"]) and os.listdir(lean["predictions"]) == []
    stats = lean["stats"]
    assert stats["encoder_calls"] >= 3 and stats["encoder_calls"] == switch_off["stats"]["encoder_calls"]
    assert stats["device_selected_calls"] == stats["encoder_calls"] and stats["host_selected_calls"] == 0
    assert stats.get("host_form_intervals", 0) == 0 and stats["fused_select"] > 0 and "fused_forward" not in stats


def test_frequency_admission_reaches_a_vcf(job, tmp_path, monkeypatch):  # noqa: F811
    """Thresholds few probabilities reach, and report_*_above_freq > 0: rows that only their frequency admits are in the VCFs."""
    high = dict(snp_p_value=0.9, insert_p_value=0.9, delete_p_value=0.9, snp_p_value_in_lc=0.95, insert_p_value_in_lc=0.95,
                delete_p_value_in_lc=0.95)
    off = _run(job, str(tmp_path / "off"), monkeypatch, freq=0.2, **high)
    lean = _run(job, str(tmp_path / "lean"), monkeypatch, freq=0.2, device_selection=True, **high)
    _same_vcfs(lean, off)
    plain = _run(job, str(tmp_path / "plain"), monkeypatch, device_selection=True, **high)
    print("totals", off["totals"], plain["totals"])
    assert off["totals"][0] > plain["totals"][0] > 0            # rows that only the frequency admits, and rows the probability does
    assert lean["stats"]["device_selected_calls"] == lean["stats"]["encoder_calls"]


def test_host_clipped_groups_are_selected_on_the_host(job, switch_off, tmp_path, monkeypatch):  # noqa: F811
    """An injected BAM handler: every group takes the host-clipped form, is selected the present way, and the run completes
    with the same VCFs."""
    from pepper_amd.variant.bam import BAM_handler
    lean = _run(job, str(tmp_path / "injected"), monkeypatch, device_selection=True, bam_handler_factory=lambda path: BAM_handler(path))
    print({k: lean["stats"].get(k) for k in COUNTS})
    assert lean["stats"]["host_selected_calls"] > 0 and lean["stats"]["device_selected_calls"] == 0
    assert lean["stats"]["host_form_intervals"] > 0
    _same_vcfs(lean, switch_off)
    assert os.listdir(lean["images"]) == [] and os.listdir(lean["predictions"]) == []


def test_switch_without_fused_inference_raises(job, tmp_path, monkeypatch):  # noqa: F811
    with pytest.raises(ValueError, match="fused_inference"):
        _run(job, str(tmp_path / "unfused"), monkeypatch, device_selection=True, fused_inference=False)
    monkeypatch.delenv("PEPPER_AMD_FUSED_CALL_VARIANT", raising=False)
    with pytest.raises(ValueError, match="fused_inference"):
        _run(job, str(tmp_path / "unfused_env"), monkeypatch, env="1", fused_inference=False)
