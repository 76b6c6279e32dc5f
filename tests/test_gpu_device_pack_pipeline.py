"""The read and pair tables built on the device (PackedEncoder.pack_device(device_pack=True), PEPPER_AMD_DEVICE_PACK=1) through
the whole image path: pack_device + encode(resident=True) against the host packer's pack + encode on every key, the
image-generation driver's files and the fused call_variant's VCFs with the switch on against the same runs with it off."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pileup_utils as pu
from pepper_amd import synthetic
from test_gpu_device_sampling import VCFS, _clean, _same_groups, _variant_groups, _variant_options, _write
from test_gpu_long_cigars import AUX_EVERY_TYPE, PARAMS, _same_outputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """A 60 kb contig in intervals of 5 kb: a few hundred reads of 0.5 - 6 kb, a pile of 300 short reads on 21 - 22 kb (over
    the sampling cap used below), CG records as the first and the last record and every sixth in between."""
    tmp = tmp_path_factory.mktemp("device_pack_job")
    rng = np.random.default_rng(5107)
    ref = pu.random_reference(rng, 60000)
    sites = {int(p): ("ACGT"[("ACGT".index(ref[p]) + 1) % 4], 0.5) for p in rng.choice(np.arange(300, 59000), 150, replace=False)}
    indels = {20000: ("I", "ACGTACGTTTGACA", 0.5), 30000: ("D", 12, 0.5)}
    reads = _clean(pu.simulate_reads(rng, ref, 0, n_reads=700, read_len=(500, 6000), snp_sites=sites, indel_sites=indels, clip_rate=0.3))
    reads += _clean(pu.simulate_reads(rng, ref[21000:22200], 21000, n_reads=300, read_len=(200, 500), snp_sites=sites))
    reads.sort(key=lambda r: r["pos"])
    plain = [dict(r) for r in reads]
    n_cg = 0
    for i, r in enumerate(reads):
        if i % 6 == 0 or i == len(reads) - 1:
            r["long_cigar"] = True
            r["aux"] = AUX_EVERY_TYPE if n_cg % 2 == 0 else b""
            n_cg += 1
    assert reads[0].get("long_cigar") and reads[-1].get("long_cigar")
    cg_dir, plain_dir = tmp / "cg", tmp / "plain"
    cg_dir.mkdir()
    plain_dir.mkdir()
    bam_cg, fa = _write(cg_dir, [("ctg", ref)], reads)
    bam, fa = _write(plain_dir, [("ctg", ref)], plain)
    sd = synthetic.variant_state_dict(seed=96, gain=2.5)
    model = str(tmp / "model.pkl")
    torch.save(synthetic.checkpoint_dict({k: torch.from_numpy(v) for k, v in sd.items()}, hidden_size=128), model)
    return SimpleNamespace(bam=bam, bam_cg=bam_cg, fasta=fa, model=model, ref=ref)


@pytest.mark.parametrize("mode", ["sampling", "long_cigars", "device_candidates"])
def test_pack_device_and_encode_equal_the_host_packer(job, mode):
    from pepper_amd.variant.bam import BAM_handler
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    edges = list(range(5000, 56000, 5000))
    starts, stops = [a - 100 for a in edges[:-1]], [b + 100 for b in edges[1:]]
    regions = list(zip(starts, stops))
    refs = [job.ref[a:b + 1] for a, b in regions]
    cands = list(zip(edges[:-1], edges[1:]))
    sampling = (7, 120, 1.0) if mode == "sampling" else None
    long_cigars = mode == "long_cigars"
    handler = BAM_handler(job.bam_cg if long_cigars else job.bam)
    enc = PackedEncoder(0, arena_bytes=64 << 20)
    enc.set_device_candidates(mode == "device_candidates")
    n_done, rp_h, counts_h = enc.pack(handler, "ctg", starts, stops, False, 1)
    assert n_done == len(starts)
    want, live_h = enc.encode(regions, refs, rp_h, counts_h, PARAMS, cands, sampling=sampling)
    if sampling:
        assert int(np.diff(rp_h).max()) > sampling[1] and enc.sampled()[0] >= 1
    laps = {}
    on_device = enc.pack_device(handler, "ctg", starts, stops, False, 1, laps=laps, long_cigars=long_cigars, device_pack=True)
    assert on_device is not None and enc.device_packed and "bam_walk_device" in laps and "bam_walk" not in laps
    n_done, rp_d, counts_d = on_device
    assert n_done == len(starts) and tuple(counts_d[:2]) == tuple(counts_h[:2]) and rp_d.tolist() == rp_h.tolist()
    # the cap that keeps the comparison from passing through a fallback: no host walk, nothing handed back
    assert enc.host_walk_spans == 0 and enc.pack_handbacks == 0 and enc.pack_calls() == (1, 0) and enc.seq_off is None
    if long_cigars:
        assert enc.long_cigar_reads > 30
    got, live_d = enc.encode(regions, refs, rp_d, counts_d, PARAMS, cands, resident=True, sampling=sampling)
    assert live_d.tolist() == live_h.tolist()
    _same_outputs(got, want)
    assert sum(len(g["candidates"]) for g in want) > 50
    if mode == "device_candidates":
        assert enc.candidate_calls() == (2, 0)
    # and the host form again on the same handle: the object remembers which form its last pack took
    n_done, rp_h2, counts_h2 = enc.pack(handler, "ctg", starts, stops, False, 1)
    assert not enc.device_packed
    again, _ = enc.encode(regions, refs, rp_h2, counts_h2, PARAMS, cands, sampling=sampling)
    _same_outputs(again, want)
    enc.close()


COUNTS = ("encoder_calls", "device_packed_calls", "host_packed_calls", "host_form_intervals")


def _generate(monkeypatch, job, out, on, threads):
    from pepper_amd.variant.ImageGenerationUI import ImageGenerationUtils
    monkeypatch.setenv("PEPPER_AMD_DEVICE_PACK", "1" if on else "0")
    stats = {}
    ImageGenerationUtils.generate_images(_variant_options(job.bam, job.fasta, out, region_size=5000, threads=threads, stage_seconds=stats))
    return _variant_groups(out), stats


@pytest.mark.parametrize("threads", [1, 3])
def test_image_files_equal_and_every_call_packed_on_the_device(job, tmp_path, monkeypatch, threads):
    got, stats = _generate(monkeypatch, job, str(tmp_path / "on"), True, threads)
    want, stats_off = _generate(monkeypatch, job, str(tmp_path / "off"), False, threads)
    print("on", {k: stats.get(k) for k in COUNTS}, "off", {k: stats_off.get(k) for k in COUNTS})
    assert _same_groups(got, want) > 100
    assert stats["encoder_calls"] >= threads and stats.get("host_form_intervals", 0) == 0
    assert stats["device_packed_calls"] == stats["encoder_calls"] == stats_off["encoder_calls"]
    assert stats["host_packed_calls"] == 0 and "bam_walk_device" in stats
    assert stats_off["device_packed_calls"] == 0 and stats_off["host_packed_calls"] == stats_off["encoder_calls"]


def test_fused_call_variant_vcfs_identical(job, tmp_path, monkeypatch):
    from pepper_amd.variant import bgzf
    from pepper_amd.variant.CallVariant import call_variant
    monkeypatch.setenv("PEPPER_AMD_BATCH_INVARIANT", "1")

    def run(out, on):
        monkeypatch.setenv("PEPPER_AMD_DEVICE_PACK", "1" if on else "0")
        stats = {}
        o = _variant_options(
            job.bam, job.fasta, None, region=None, region_size=5000, threads=3, output_dir=out, fused_inference=True,
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
    assert stats["encoder_calls"] >= 3 and stats.get("host_form_intervals", 0) == 0
    assert stats["device_packed_calls"] == stats["encoder_calls"] == stats_off["encoder_calls"]
    assert stats["host_packed_calls"] == 0 and stats_off["device_packed_calls"] == 0
    for name in VCFS:
        assert len(got[name]) == len(want[name]), name
        for g, w in zip(got[name], want[name]):
            assert g == w, (name, g, w)
