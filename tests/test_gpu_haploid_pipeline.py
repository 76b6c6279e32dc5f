"""options.haploid_contigs / options.par_regions_bed through call_variant: the three-step run, the fused run and the fused run
with the device selection write the same files, haploid where asked and untouched elsewhere.

Two contigs of 20 kb at ~40x in intervals of 4 kb (built with the helpers of tests/test_gpu_region_bed_pipeline.py): ctgA
diploid, ctgH haploid with a PAR on 6 500 - 10 500, which cuts through the intervals on 4 - 8 kb and 8 - 12 kb.  SNPs are planted
on both PAR edges (6 499 / 6 500, 10 499 / 10 500) and on the interval boundaries at 4 000, 8 000 (inside the PAR) and 12 000, and
sites where half the reads carry one alternative base and half another -- two-allele sites -- on ctgA, inside the PAR and
outside it."""
import gzip
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bam_utils as bu
import pileup_utils as pu
from pepper_amd import synthetic
from pepper_amd.variant import Gvcf, bgzf
from test_gpu_device_sampling import VCFS, _clean, _variant_options

pytestmark = pytest.mark.gpu

REGION_SIZE = 4000
LENGTH = 20000
PAR = (6500, 10500)
MODEL_SEED = 42                      # (a synthetic model whose feature-off run has the het records the test asks for, below;
#                                      seed 96 of the region_bed job calls nearly every site 1/1 here)
TWO_ALLELE = {"ctgA": (3100, 15100), "ctgH": (2100, 7300, 9100, 14100, 17100)}      # 7 300 and 9 100 lie inside the PAR
FORMS = {"three_step": {}, "fused": dict(fused_inference=True), "fused_device_selection": dict(fused_inference=True, device_selection=True)}


def _haploid(contig, pos0):
    return contig == "ctgH" and not PAR[0] <= pos0 < PAR[1]


def build_job(tmp):
    rng = np.random.default_rng(5113)
    refs, by_tid = [], {}
    for tid, contig in enumerate(("ctgA", "ctgH")):
        ref = pu.random_reference(rng, LENGTH, n_frac=0.001)

        def other(p, step=1):
            return "ACGT"[(("ACGT".index(ref[p]) if ref[p] in "ACGT" else 0) + step) % 4]
        sites = {int(p): (other(int(p)), 0.5) for p in rng.choice(np.arange(300, LENGTH - 500), 130, replace=False)}
        for p in (4000, 6499, 6500, 8000, 10499, 10500, 12000):
            sites[p] = (other(p), 0.5)
        indels = {5100: ("I", "ACGTTGACA", 0.5), 9000: ("D", 6, 0.5), 13000: ("I", "TT", 0.6), 16000: ("D", 4, 0.5)}
        reads = []
        for step in (1, 2):              # two halves of the reads: at a two-allele site each half carries a base of its own
            mine = dict(sites)
            for p in TWO_ALLELE[contig]:
                mine[p] = (other(p, step), 0.9)
            reads += _clean(pu.simulate_reads(rng, ref, 0, n_reads=200, read_len=(500, 4000), snp_sites=mine, indel_sites=indels,
                                              clip_rate=0.3))
        reads.sort(key=lambda r: r["pos"])
        for i, r in enumerate(reads):
            r["name"] = "q%d_%d" % (tid, i)
        refs.append((contig, ref))
        by_tid[tid] = reads
    bam, fa = str(tmp / "in.bam"), str(tmp / "in.fa")
    bu.write_bam(bam, [(n, len(s)) for n, s in refs], by_tid, flush_every=47)
    with open(fa, "w") as fh:
        for n, s in refs:
            fh.write(">" + n + "\n" + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    sd = synthetic.variant_state_dict(seed=MODEL_SEED, gain=2.5)
    model = str(tmp / "model.pkl")
    torch.save(synthetic.checkpoint_dict({k: torch.from_numpy(v) for k, v in sd.items()}, hidden_size=128), model)
    par = str(tmp / "par.bed")
    with open(par, "w") as fh:
        fh.write("ctgH\t%d\t%d\nctgA\t100\t900\n" % PAR)
    return SimpleNamespace(bam=bam, fasta=fa, model=model, par=par)


def call_variant(job, out, form, haploid, **over):
    from pepper_amd.variant.CallVariant import call_variant as run
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PEPPER_AMD_BATCH_INVARIANT", "1")
        mp.setenv("PEPPER_AMD_PACKED_READS", "1")
        mp.setenv("PEPPER_AMD_DEVICE_CANDIDATES", "0")
        for key in ("PEPPER_AMD_DEVICE_SELECTION", "PEPPER_AMD_FUSED_CALL_VARIANT", "PEPPER_AMD_GVCF", "PEPPER_AMD_HAPLOID_CONTIGS",
                    "PEPPER_AMD_PAR_REGIONS_BED", "PEPPER_AMD_CANDIDATES_PYTHON", "PEPPER_AMD_CANDIDATES_TUPLES"):
            mp.delenv(key, raising=False)
        stats = {}
        o = _variant_options(
            job.bam, job.fasta, None, region=None, region_size=REGION_SIZE, threads=3, output_dir=out,
            model_path=job.model, batch_size=128, num_workers=0, gpu=True, device_ids="0", callers_per_gpu=1,
            quantized=False, dry=False, sample_name="SYN", allowed_multiallelics=4,
            snp_p_value=0.1, insert_p_value=0.25, delete_p_value=0.25, snp_p_value_in_lc=0.1,
            insert_p_value_in_lc=0.3, delete_p_value_in_lc=0.3, snp_q_cutoff=20, indel_q_cutoff=15,
            snp_q_cutoff_in_lc=20, indel_q_cutoff_in_lc=10, report_snp_above_freq=0, report_indel_above_freq=0,
            stage_seconds=stats, **FORMS[form], **over)
        del o.image_output_directory
        if haploid:                                        # (off: the attributes do not exist, as in every other test's options)
            o.haploid_contigs = "ctgH"
            o.par_regions_bed = job.par
        run(o)
    vcfs = {name: bgzf.read_bgzf(os.path.join(out, name + ".vcf.gz")).decode().splitlines() for name in VCFS}
    index = {name: bgzf.read_bgzf(os.path.join(out, name + ".vcf.gz.tbi")) for name in VCFS}
    return SimpleNamespace(vcfs=vcfs, index=index, stats=stats, out=out)


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    return build_job(tmp_path_factory.mktemp("haploid_job"))


@pytest.fixture(scope="module")
def runs(job, tmp_path_factory):
    made = {form: call_variant(job, str(tmp_path_factory.mktemp("haploid_" + form)), form, True) for form in FORMS}
    made["off"] = call_variant(job, str(tmp_path_factory.mktemp("haploid_off")), "fused_device_selection", False)
    return made


def _data(lines):
    return [line.split("\t") for line in lines if not line.startswith("#")]


def _gt(fields):
    return fields[9].split(":")[0]


def genotype_counts(lines):
    """{(where, GT): records} of a VCF's data lines; where: ctgA, par, haploid."""
    out = {}
    for f in _data(lines):
        where = "ctgA" if f[0] == "ctgA" else ("haploid" if _haploid(f[0], int(f[1]) - 1) else "par")
        out[where, _gt(f)] = out.get((where, _gt(f)), 0) + 1
    return out


def test_the_comparison_is_not_vacuous(runs):
    off = runs["off"].vcfs["PEPPER_VARIANT_FULL"]
    counts = genotype_counts(off)
    print("feature off:", sorted(counts.items()))
    print("feature on: ", sorted(genotype_counts(runs["fused_device_selection"].vcfs["PEPPER_VARIANT_FULL"]).items()))
    assert counts.get(("haploid", "0/1"), 0) >= 10
    assert counts.get(("par", "0/1"), 0) >= 3
    # the two-allele site on the haploid stretch is there: two ALTs, one number for a genotype
    on = {(f[0], int(f[1]) - 1): f for f in _data(runs["fused_device_selection"].vcfs["PEPPER_VARIANT_FULL"])}
    two = [on[("ctgH", p)] for p in TWO_ALLELE["ctgH"] if _haploid("ctgH", p) and ("ctgH", p) in on and "," in on["ctgH", p][4]]
    print("two-allele haploid sites:", [(f[1], f[4], f[9]) for f in two])
    assert two and all(_gt(f) in ("0", "1", "2") for f in two)
    # ... and so is one that stays diploid
    assert any("," in f[4] for key, f in on.items() if not _haploid(*key))


def test_three_forms_write_the_same_files(runs):
    want = runs["three_step"]
    assert sum(1 for _ in _data(want.vcfs["PEPPER_VARIANT_FULL"])) >= 60
    for form in ("fused", "fused_device_selection"):
        for name in VCFS:
            assert runs[form].vcfs[name] == want.vcfs[name], (form, name)
            assert runs[form].index[name] == want.index[name], (form, name)
    stats = runs["fused_device_selection"].stats
    print({k: stats.get(k) for k in ("encoder_calls", "device_selected_calls", "host_selected_calls")})
    assert stats["host_selected_calls"] == 0 and stats["device_selected_calls"] == stats["encoder_calls"] >= 3


def test_haploid_outside_the_par_and_untouched_elsewhere(runs):
    on, off = runs["fused_device_selection"].vcfs, runs["off"].vcfs
    for name in VCFS:
        rows = _data(on[name])
        outside = [f for f in rows if _haploid(f[0], int(f[1]) - 1)]
        assert all("/" not in _gt(f) for f in outside), name
        unchanged = lambda lines: [f for f in _data(lines) if not _haploid(f[0], int(f[1]) - 1)]      # noqa: E731
        assert unchanged(on[name]) == unchanged(off[name]), name
        head = [line for line in on[name] if line.startswith("#")]
        off_head = [line for line in off[name] if line.startswith("#")]
        assert head[6] == "##pepper_amd_haploid_contigs=ctgH;par_regions_bed=par.bed" and head[:6] + head[7:] == off_head
    full = _data(on["PEPPER_VARIANT_FULL"])
    assert len([f for f in full if _haploid(f[0], int(f[1]) - 1)]) >= 20
    # the planted SNPs on the PAR edges: haploid at 6 499 and 10 500, diploid at 6 500 and 10 499
    by_pos = {int(f[1]) - 1: _gt(f) for f in full if f[0] == "ctgH"}
    seen = {p: by_pos.get(p) for p in (6499, 6500, 10499, 10500)}
    print("PAR edges:", seen)
    assert all(("/" in gt) == (PAR[0] <= p < PAR[1]) for p, gt in seen.items() if gt is not None)
    assert sum(gt is not None for gt in seen.values()) >= 2


def test_gvcf_blocks_follow_the_ploidy(job, runs, tmp_path):
    got = call_variant(job, str(tmp_path / "gvcf"), "fused_device_selection", True, gvcf=True)
    for name in VCFS:
        assert got.vcfs[name] == runs["fused_device_selection"].vcfs[name], name
    with gzip.open(os.path.join(got.out, Gvcf.GVCF_NAME), "rb") as fh:
        lines = fh.read().decode().splitlines()
    rows = _data(lines)
    records = [f for f in rows if f[4] != "<NON_REF>"]
    blocks = [(f[0], int(f[1]) - 1, int(f[7][4:]), _gt(f), int(f[9].split(":")[2])) for f in rows if f[4] == "<NON_REF>"]
    assert records == _data(got.vcfs["PEPPER_VARIANT_FULL"]) and len(blocks) > 50
    seen = set()
    for contig, start, end, gt, min_dp in blocks:
        haploid = _haploid(contig, start)
        assert haploid == _haploid(contig, end - 1), (contig, start, end)            # cut at the PAR edges
        assert gt == (("0" if min_dp > 0 else ".") if haploid else ("0/0" if min_dp > 0 else "./.")), (contig, start, end)
        seen.add((contig, haploid, gt))
    assert {("ctgA", False, "0/0"), ("ctgH", False, "0/0"), ("ctgH", True, "0")} <= seen
    # a block ends and one begins on each PAR edge unless a record lies there
    on_record = lambda p: any(f[0] == "ctgH" and int(f[1]) - 1 <= p < int(f[1]) - 1 + len(f[3]) for f in records)      # noqa: E731
    for edge in PAR:
        assert on_record(edge - 1) or any(c == "ctgH" and e == edge for c, _s, e, _g, _d in blocks)
        assert on_record(edge) or any(c == "ctgH" and s == edge for c, s, _e, _g, _d in blocks)
