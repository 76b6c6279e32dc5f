"""The image-generation driver and the fused call_variant with PEPPER_AMD_DEVICE_CANDIDATES=1 against the same runs with =0
(candidates enumerated on the host, which tests/test_gpu_packed.py holds to the host-clipped form and that to the reference's
build): image files equal dataset by dataset with one worker and with three, every encoder call counted as enumerated on the
device, VCFs identical line for line."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pileup_utils as pu
from pepper_amd import synthetic
from test_gpu_device_sampling import VCFS, _clean, _same_groups, _variant_groups, _variant_options, _write

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """A 40 kb contig at ~45x in intervals of 4 kb: SNPs, short indels, two inserts of 14 bases that agree on their first 8 (the
    pool), a deletion of 12, and a pile of 700 short reads on 21 - 22 kb (sites of several hundred votes)."""
    tmp = tmp_path_factory.mktemp("device_candidates_job")
    rng = np.random.default_rng(4021)
    ref = pu.random_reference(rng, 40000, n_frac=0.001)
    sites = {int(p): ("ACGT"[(("ACGT".index(ref[p]) if ref[p] in "ACGT" else 0) + 1) % 4], 0.5)
             for p in rng.choice(np.arange(300, 39500), 160, replace=False)}
    indels = {5100: ("I", "ACGTACGTTTGACA", 0.4), 9000: ("D", 12, 0.5), 21400: ("I", "CAG", 0.5), 21600: ("D", 4, 0.5),
              30000: ("I", "TT", 0.6)}
    reads = _clean(pu.simulate_reads(rng, ref, 0, n_reads=1000, read_len=(500, 4000), snp_sites=sites, indel_sites=indels, clip_rate=0.3))
    reads += _clean(pu.simulate_reads(rng, ref[21000:22200], 21000, n_reads=700, read_len=(200, 500), snp_sites=sites, indel_sites=indels))
    for r in reads:                                    # the twin of the long insert: the same first 8 bytes, another tail
        if r["pos"] < 5000 and rng.random() < 0.5:
            r["seq"] = r["seq"].replace("ACGTACGTTTGACA", "ACGTACGAAAAAAA", 1)
    bam, fa = _write(tmp, [("ctg", ref)], reads)
    sd = synthetic.variant_state_dict(seed=96, gain=2.5)
    model = str(tmp / "model.pkl")
    torch.save(synthetic.checkpoint_dict({k: torch.from_numpy(v) for k, v in sd.items()}, hidden_size=128), model)
    return SimpleNamespace(bam=bam, fasta=fa, model=model)


COUNTS = ("encoder_calls", "device_enumerated_calls", "host_enumerated_calls", "host_form_intervals")


def _generate(monkeypatch, job, out, on, threads):
    from pepper_amd.variant.ImageGenerationUI import ImageGenerationUtils
    monkeypatch.setenv("PEPPER_AMD_DEVICE_CANDIDATES", "1" if on else "0")
    stats = {}
    ImageGenerationUtils.generate_images(_variant_options(job.bam, job.fasta, out, region_size=4000, threads=threads, stage_seconds=stats))
    return _variant_groups(out), stats


@pytest.mark.parametrize("threads", [1, 3])
def test_image_files_equal_and_every_call_on_the_device(job, tmp_path, monkeypatch, threads):
    got, stats = _generate(monkeypatch, job, str(tmp_path / "on"), True, threads)
    want, stats_off = _generate(monkeypatch, job, str(tmp_path / "off"), False, threads)
    print("on", {k: stats.get(k) for k in COUNTS}, "off", {k: stats_off.get(k) for k in COUNTS})
    assert _same_groups(got, want) > 150
    assert any(len(c[0]) > 10 for g in got.values() for c in g["candidates"])          # the pooled alleles are among them
    # every worker has intervals, so every worker's handle made calls: each of them enumerated on the device, none handed back,
    # and as many calls as the same job makes with the switch off
    assert stats["encoder_calls"] >= threads and stats.get("host_form_intervals", 0) == 0
    assert stats["device_enumerated_calls"] == stats["encoder_calls"] == stats_off["encoder_calls"]
    assert stats["host_enumerated_calls"] == 0
    assert stats_off["device_enumerated_calls"] == 0 and stats_off["host_enumerated_calls"] == 0 and "encode" in stats_off


def test_fused_call_variant_vcfs_identical(job, tmp_path, monkeypatch):
    from pepper_amd.variant import bgzf
    from pepper_amd.variant.CallVariant import call_variant
    monkeypatch.setenv("PEPPER_AMD_BATCH_INVARIANT", "1")

    def run(out, on):
        monkeypatch.setenv("PEPPER_AMD_DEVICE_CANDIDATES", "1" if on else "0")
        stats = {}
        o = _variant_options(
            job.bam, job.fasta, None, region=None, region_size=4000, threads=3, output_dir=out, fused_inference=True,
            model_path=job.model, batch_size=128, num_workers=0, gpu=True, device_ids="0", callers_per_gpu=1,
            quantized=False, dry=False, sample_name="SYN", allowed_multiallelics=4,
            snp_p_value=0.1, insert_p_value=0.25, delete_p_value=0.25, snp_p_value_in_lc=0.1,
            insert_p_value_in_lc=0.3, delete_p_value_in_lc=0.3, snp_q_cutoff=20, indel_q_cutoff=15,
            snp_q_cutoff_in_lc=20, indel_q_cutoff_in_lc=10, report_snp_above_freq=0, report_indel_above_freq=0,
            stage_seconds=stats)
        del o.image_output_directory
        _, _, totals = call_variant(o)
        return totals, stats, {name: bgzf.read_bgzf(os.path.join(out, name + ".vcf.gz")).decode().splitlines() for name in VCFS}
    totals, stats, got = run(str(tmp_path / "on"), True)
    totals_off, stats_off, want = run(str(tmp_path / "off"), False)
    print("on", {k: stats.get(k) for k in COUNTS}, "off", {k: stats_off.get(k) for k in COUNTS})
    assert totals == totals_off and totals[0] > 30
    # the fused run passed the variable on: its workers' calls were enumerated on the device, every one of them
    assert stats["encoder_calls"] >= 3 and stats.get("host_form_intervals", 0) == 0
    assert stats["device_enumerated_calls"] == stats["encoder_calls"] == stats_off["encoder_calls"]
    assert stats["host_enumerated_calls"] == 0
    assert stats_off["device_enumerated_calls"] == 0 and stats_off["host_enumerated_calls"] == 0
    for name in VCFS:
        assert len(got[name]) == len(want[name]), name
        for g, w in zip(got[name], want[name]):
            assert g == w, (name, g, w)
