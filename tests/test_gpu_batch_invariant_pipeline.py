"""Batch-invariant mode through the pipelines: call_variant(options.batch_invariant=True) and polish(batch_invariant=True)
give byte-identical outputs whatever the form of the run -- three-step or fused, one caller or two on the device, the
batch size, the reader lanes.  The comparisons here are strict: no tolerance anywhere."""
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pepper_amd import h5, synthetic

pytestmark = pytest.mark.gpu

VCFS = ("PEPPER_VARIANT_FULL", "PEPPER_VARIANT_OUTPUT_PEPPER", "PEPPER_VARIANT_OUTPUT_VARIANT_CALLING",
        "PEPPER_VARIANT_OUTPUT_VARIANT_CALLING_SNPs", "PEPPER_VARIANT_OUTPUT_VARIANT_CALLING_INDEL")


def _vcf_lines(d):
    from pepper_amd.variant import bgzf
    return {name: bgzf.read_bgzf(os.path.join(d, name + ".vcf.gz")).decode().splitlines() for name in VCFS}


def _assert_identical_vcfs(got_dir, want_dir):
    got, want = _vcf_lines(got_dir), _vcf_lines(want_dir)
    for name in VCFS:
        assert len(got[name]) == len(want[name]), name
        for g, w in zip(got[name], want[name]):
            assert g == w, (name, g, w)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    import bam_utils as bu
    import pileup_utils as pu
    tmp = tmp_path_factory.mktemp("bi_inputs")
    rng = np.random.default_rng(707)
    ref = pu.random_reference(rng, 7000)
    sites = {int(p): ("ACGT"[(("ACGT".index(ref[p]) + 1) % 4)], 0.5) for p in rng.choice(np.arange(200, 6800), 40, replace=False)}
    indels = {900: ("I", "CA", 0.6), 2500: ("D", 2, 0.7), 5100: ("D", 9, 0.5)}
    reads = pu.simulate_reads(rng, ref, 0, n_reads=520, read_len=(400, 1800), snp_sites=sites, indel_sites=indels)
    reads = sorted([r for r in reads if not any(op in (3, 6) for op, _ in r["cigar"])], key=lambda r: r["pos"])
    for i, r in enumerate(reads):
        r["name"] = "q%d" % i
    bam_path, fa_path = str(tmp / "in.bam"), str(tmp / "ref.fa")
    bu.write_bam(bam_path, [("chr20", len(ref))], {0: reads}, flush_every=50)
    with open(fa_path, "w") as fh:
        fh.write(">chr20\n" + "\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + "\n")
    sd = synthetic.variant_state_dict(seed=94, gain=2.5)
    vmodel = str(tmp / "model.pkl")
    torch.save(synthetic.checkpoint_dict({k: torch.from_numpy(v) for k, v in sd.items()}, hidden_size=128), vmodel)
    psd = synthetic.polish_state_dict(seed=19, gain=2.0)
    pmodel = str(tmp / "polish.pkl")
    torch.save(synthetic.checkpoint_dict({k: torch.from_numpy(v) for k, v in psd.items()}, hidden_size=128), pmodel)
    return SimpleNamespace(bam=bam_path, fasta=fa_path, vmodel=vmodel, pmodel=pmodel)


def _variant_options(inp, out, **over):
    o = dict(
        bam=inp.bam, fasta=inp.fasta, region=None, region_size=1500, threads=4, train_mode=False,
        use_hp_info=False, include_supplementary=False, output_dir=out,
        min_mapq=1, min_snp_baseq=1, min_indel_baseq=1, snp_frequency=0.10, insert_frequency=0.15,
        delete_frequency=0.15, min_coverage_threshold=3, snp_candidate_frequency_threshold=0.10,
        indel_candidate_frequency_threshold=0.12, candidate_support_threshold=2, skip_indels=False,
        downsample_rate=1.0,
        model_path=inp.vmodel, batch_size=512, num_workers=0, gpu=True, device_ids="0", callers_per_gpu=1,
        quantized=False, dry=False, sample_name="SYN", allowed_multiallelics=4,
        snp_p_value=0.1, insert_p_value=0.25, delete_p_value=0.25, snp_p_value_in_lc=0.1,
        insert_p_value_in_lc=0.3, delete_p_value_in_lc=0.3, snp_q_cutoff=20, indel_q_cutoff=15,
        snp_q_cutoff_in_lc=20, indel_q_cutoff_in_lc=10, report_snp_above_freq=0, report_indel_above_freq=0,
        batch_invariant=True)
    o.update(over)
    return SimpleNamespace(**o)


def test_call_variant_vcfs_identical_across_run_forms(inputs, tmp_path):
    from pepper_amd.variant.CallVariant import call_variant
    base = str(tmp_path / "base")
    _, _, totals = call_variant(_variant_options(inputs, base))
    assert totals[0] > 20
    forms = {"fused": dict(fused_inference=True), "two_callers": dict(device_ids="0,0"), "batch_64": dict(batch_size=64),
             "lanes": dict(num_workers=2)}
    for name, over in forms.items():
        out = str(tmp_path / name)
        _, _, t = call_variant(_variant_options(inputs, out, **over))
        assert t == totals, name
        _assert_identical_vcfs(out, base)


def _predictions(directory):
    """{(group path, chunk): (bases, phred_score)} over every prediction store of a directory."""
    out = {}

    def walk(f, path):
        try:
            keys = f.keys(path)
        except Exception:
            return
        if "bases" in keys and "phred_score" in keys:
            out[path] = (np.array(f[path + "/bases"]), np.array(f[path + "/phred_score"]))
            return
        for k in keys:
            walk(f, path + "/" + k)

    for name in sorted(glob.glob(os.path.join(directory, "*.hdf"))):
        with h5.File(name) as f:
            walk(f, "predictions")
    return out


def test_polish_identical_across_run_forms(inputs, tmp_path):
    from pepper_amd.polish.polish import polish
    runs = {}
    for name, device_ids, fused in (("three_step", "0", False), ("fused", "0", True), ("two_callers", "0,0", False)):
        out_dir = str(tmp_path / name) + "/"
        polish(inputs.bam, inputs.fasta, out_dir, 4, None, inputs.pmodel, 64, True, device_ids, 0, fused_inference=fused,
               batch_invariant=True)
        fasta = glob.glob(out_dir + "*.fa")
        assert len(fasta) == 1
        preds = {}
        for d in glob.glob(out_dir + "predictions_*"):
            preds.update(_predictions(d))
        runs[name] = (open(fasta[0]).read(), preds)
    text, preds = runs["three_step"]
    assert text.startswith(">chr20") and len(preds) > 0
    for name in ("fused", "two_callers"):
        t, p = runs[name]
        assert t == text, name
        # (which store a chunk lands in may differ; the chunk's group path does not)
        assert set(p) == set(preds), name
        for k in preds:
            assert np.array_equal(p[k][0], preds[k][0]) and np.array_equal(p[k][1], preds[k][1]), (name, k)
