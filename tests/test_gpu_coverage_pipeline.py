"""options.coverage_bed through the image-generation driver and call_variant: PEPPER_VARIANT_COVERAGE.bed against the numpy rule
over the whole BAM (coverage_cases.depth_numpy + Coverage.runs_numpy; nothing expected comes from the code under test).

The job of tests/test_gpu_region_bed_pipeline.py -- a 40 kb contig at ~45x in intervals of 4 kb, a pile of short reads on
21 - 22 kb, the same BED -- with two holes cut into the reads: nothing overlaps 13 000 - 15 000 (NO_COVERAGE inside an interval,
LOW_COVERAGE on its slopes), and nothing overlaps 23 900 - 28 100, the whole fetch range of the interval 24 000 - 28 000, which
therefore has no read at all and still reports its run."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bam_utils as bu
import pileup_utils as pu
from coverage_cases import depth_numpy
from pepper_amd import synthetic
from pepper_amd.variant import Coverage, Targets
from test_gpu_device_sampling import VCFS, _clean, _variant_options, _write
from test_gpu_region_bed_pipeline import BED_TEXT, DROPPED, KEPT, REGION_SIZE

pytestmark = pytest.mark.gpu

LENGTH = 40000
HOLES = [(13000, 15000), (23900, 28100)]
INTERVALS = [(s, min(s + REGION_SIZE, LENGTH - 1)) for s in range(0, LENGTH - 1, REGION_SIZE)]
BINS, LABELS = [0, 1, 3], ["NO_COVERAGE", "LOW_COVERAGE", "CALLABLE"]
SAFE = 100


def build_job(tmp):
    rng = np.random.default_rng(5150)
    ref = pu.random_reference(rng, LENGTH, n_frac=0.001)

    def other(p):
        return "ACGT"[(("ACGT".index(ref[p]) if ref[p] in "ACGT" else 0) + 1) % 4]
    sites = {int(p): (other(int(p)), 0.5) for p in rng.choice(np.arange(300, 39500), 260, replace=False)}
    for p in (8000, 20000, 21300):
        sites[p] = (other(p), 0.5)
    indels = {5100: ("I", "ACGTACGTTTGACA", 0.4), 9000: ("D", 12, 0.5), 21400: ("I", "CAG", 0.5), 30000: ("I", "TT", 0.6)}
    reads = _clean(pu.simulate_reads(rng, ref, 0, n_reads=1000, read_len=(500, 4000), snp_sites=sites, indel_sites=indels, clip_rate=0.3))
    reads += _clean(pu.simulate_reads(rng, ref[21000:22200], 21000, n_reads=700, read_len=(200, 500), snp_sites=sites, indel_sites=indels))
    reads = [r for r in reads if not any(r["pos"] < hi and r["pos"] + bu.ref_length(r["cigar"]) > lo for lo, hi in HOLES)]
    bam, fa = _write(tmp, [("ctg", ref)], reads)
    sd = synthetic.variant_state_dict(seed=96, gain=2.5)
    model = str(tmp / "model.pkl")
    torch.save(synthetic.checkpoint_dict({k: torch.from_numpy(v) for k, v in sd.items()}, hidden_size=128), model)
    bed = str(tmp / "targets.bed")
    with open(bed, "w") as fh:
        fh.write(BED_TEXT)
    table = Targets.read_bed(bed, {"ctg": len(ref)})["ctg"]
    return SimpleNamespace(bam=bam, fasta=fa, model=model, bed=bed, table=table, reads=sorted(reads, key=lambda r: r["pos"]))


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    return build_job(tmp_path_factory.mktemp("coverage_job"))


def _bed_lines(which):
    """int per position (-1: not reported) -> the BED's lines by the numpy rule."""
    heads = np.flatnonzero(np.concatenate([[True], which[1:] != which[:-1]]))
    ends = np.concatenate([heads[1:], [len(which)]])
    return ["ctg\t%d\t%d\t%s" % (a, z, LABELS[which[a]]) for a, z in zip(heads.tolist(), ends.tolist()) if which[a] >= 0]


@pytest.fixture(scope="module")
def expected(job):
    """The whole-contig answer, interval by interval as the driver fetches: the reads with pos < end + 100 and a base behind
    start - 100 and mapping quality >= 1 (no interval has more than 5 000, so no sample is drawn), their depth over the interval,
    the position two intervals share taken from the one that starts there.  -> (lines without a BED, lines with the BED)."""
    which = np.full(LENGTH, -1, np.int64)
    for s, e in INTERVALS:
        lo, hi = max(0, s - SAFE), e + SAFE
        fetched = [r for r in job.reads if r["pos"] < hi and r["pos"] + bu.ref_length(r["cigar"]) > lo]
        assert len(fetched) < 5000
        depth = depth_numpy(fetched, s, e, 1, 1, 1)
        which[s:e + 1] = np.searchsorted(np.array(BINS), depth, side="right") - 1
    assert (which >= 0).all()
    counts = np.bincount(which, minlength=3)
    print("expected bases per class:", counts.tolist())
    assert counts[0] > 5000 and counts[1] > 20 and counts[2] > 25000
    assert (which[24000:28001] == 0).all()                           # the interval without any read
    restricted = np.full(LENGTH, -1, np.int64)
    for s, e in KEPT:
        inside = Targets.contains(job.table[0], job.table[1], np.arange(s, e + 1, dtype=np.int64))
        restricted[s:e + 1] = np.where(inside, which[s:e + 1], -1)
    for s, e in DROPPED:
        assert (restricted[s + 1:e] == -1).all()
    return _bed_lines(which), _bed_lines(restricted)


def _read_bed(directory):
    with open(os.path.join(directory, Coverage.BED_NAME)) as fh:
        return fh.read().splitlines()


def _vcfs(out):
    from pepper_amd.variant import bgzf
    return {name: bgzf.read_bgzf(os.path.join(out, name + ".vcf.gz")).decode().splitlines() for name in VCFS}


def _call_variant(monkeypatch, job, out, coverage, threads=3, bed=False, **over):
    from pepper_amd.variant.CallVariant import call_variant
    monkeypatch.setenv("PEPPER_AMD_BATCH_INVARIANT", "1")
    monkeypatch.setenv("PEPPER_AMD_PACKED_READS", "1")
    monkeypatch.setenv("PEPPER_AMD_DEVICE_CANDIDATES", "0")
    monkeypatch.delenv("PEPPER_AMD_DEVICE_SELECTION", raising=False)
    monkeypatch.delenv("PEPPER_AMD_FUSED_CALL_VARIANT", raising=False)
    monkeypatch.delenv("PEPPER_AMD_COVERAGE_BED", raising=False)
    stats = {}
    o = _variant_options(
        job.bam, job.fasta, None, region=None, region_size=REGION_SIZE, threads=threads, output_dir=out,
        model_path=job.model, batch_size=128, num_workers=0, gpu=True, device_ids="0", callers_per_gpu=1,
        quantized=False, dry=False, sample_name="SYN", allowed_multiallelics=4,
        snp_p_value=0.1, insert_p_value=0.25, delete_p_value=0.25, snp_p_value_in_lc=0.1,
        insert_p_value_in_lc=0.3, delete_p_value_in_lc=0.3, snp_q_cutoff=20, indel_q_cutoff=15,
        snp_q_cutoff_in_lc=20, indel_q_cutoff_in_lc=10, report_snp_above_freq=0, report_indel_above_freq=0,
        stage_seconds=stats, **over)
    del o.image_output_directory
    if coverage:
        o.coverage_bed = True
    if bed:
        o.region_bed = job.bed
    call_variant(o)
    return _vcfs(out), stats


FORMS = {"three_step": {}, "fused": dict(fused_inference=True), "fused_device_selection": dict(fused_inference=True, device_selection=True)}


@pytest.fixture(scope="module")
def plain_vcfs(job, tmp_path_factory):
    """The VCFs of every form without coverage_bed (threads do not change them: tests/test_gpu_fused_call_variant.py and its
    neighbours hold that), and that no BED is written then."""
    made = {}
    for form, over in FORMS.items():
        out = str(tmp_path_factory.mktemp("coverage_plain_" + form))
        with pytest.MonkeyPatch.context() as mp:
            made[form], stats = _call_variant(mp, job, out, coverage=False, **over)
        assert not os.path.exists(os.path.join(out, Coverage.BED_NAME))
        assert not any(key.startswith("coverage") for key in stats)
        assert sum(1 for line in made[form]["PEPPER_VARIANT_FULL"] if not line.startswith("#")) >= 20
    return made


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("form", list(FORMS))
def test_call_variant_writes_the_numpy_rules_bed_and_the_same_vcfs(job, expected, plain_vcfs, tmp_path, monkeypatch, form, threads):
    out = str(tmp_path / "cov")
    vcfs, stats = _call_variant(monkeypatch, job, out, coverage=True, threads=threads, **FORMS[form])
    lines = _read_bed(out)
    assert len(lines) == len(expected[0]) > 10
    assert lines == expected[0]
    for name in VCFS:
        assert vcfs[name] == plain_vcfs[form][name], name
    print(form, threads, {k: v for k, v in stats.items() if k.startswith("coverage") or k in ("encoder_calls", "host_form_intervals")})
    assert stats["coverage_overflows"] == 0 and stats.get("host_form_intervals", 0) == 0
    assert stats["coverage_calls"] == stats["encoder_calls"] >= threads and stats["coverage_runs"] >= len(lines)


def _generate(monkeypatch, job, out, packed=True, threads=1, bed=False, **over):
    from pepper_amd.variant.ImageGenerationUI import ImageGenerationUtils
    monkeypatch.setenv("PEPPER_AMD_PACKED_READS", "1" if packed else "0")
    monkeypatch.setenv("PEPPER_AMD_DEVICE_CANDIDATES", "0")
    stats = {}
    options = _variant_options(job.bam, job.fasta, out, region=None, region_size=REGION_SIZE, threads=threads, stage_seconds=stats, **over)
    if bed:
        options.region_bed = job.bed
    ImageGenerationUtils.generate_images(options)
    assert not hasattr(options, "coverage_track")
    return _read_bed(out), stats


@pytest.mark.parametrize("threads,encoder_batch", [(1, 16), (3, 2)])
def test_every_interval_host_clipped_gives_the_same_bed(job, expected, tmp_path, monkeypatch, threads, encoder_batch):
    """PEPPER_AMD_PACKED_READS=0: make_images through BAM_handler.get_reads and this thread's handle; the interval without a read
    is never encoded there and reports its run all the same."""
    lines, stats = _generate(monkeypatch, job, str(tmp_path / "host"), packed=False, threads=threads, encoder_batch=encoder_batch,
                             coverage_bed=True)
    assert lines == expected[0]
    assert stats["host_form_intervals"] == len(INTERVALS) and stats["encoder_calls"] == 0
    assert stats["coverage_overflows"] == 0 and stats["coverage_calls"] >= threads and stats["coverage_runs"] > 10


def test_the_environment_switch_and_custom_bins(job, expected, tmp_path, monkeypatch):
    monkeypatch.setenv("PEPPER_AMD_COVERAGE_BED", "1")
    lines, _ = _generate(monkeypatch, job, str(tmp_path / "env"), threads=2, encoder_batch=3)
    assert lines == expected[0]
    monkeypatch.delenv("PEPPER_AMD_COVERAGE_BED")
    lines, _ = _generate(monkeypatch, job, str(tmp_path / "bins"), coverage_bed=True, coverage_bins="0,3")
    # two classes: the default's NO_COVERAGE and LOW_COVERAGE runs merged under mosdepth's label
    want = []
    for line in expected[0]:
        contig, s, e, label = line.split("\t")
        label = "3:inf" if label == "CALLABLE" else "0:3"
        if want and want[-1][2] == s and want[-1][3] == label:
            want[-1][2] = e
        else:
            want.append([contig, s, e, label])
    assert lines == ["\t".join(w) for w in want] and any(w[3] == "0:3" for w in want)
    with pytest.raises(ValueError):
        _generate(monkeypatch, job, str(tmp_path / "bad"), coverage_bed=True, coverage_bins="0,3,3")


@pytest.mark.parametrize("packed", [True, False])
def test_with_region_bed_the_track_covers_the_targets_of_the_kept_intervals(job, expected, tmp_path, monkeypatch, packed):
    lines, stats = _generate(monkeypatch, job, str(tmp_path / "bed"), packed=packed, threads=3, bed=True, coverage_bed=True)
    assert lines == expected[1] and len(lines) >= 10
    covered = sum(int(line.split("\t")[2]) - int(line.split("\t")[1]) for line in lines)
    kept_positions = np.unique(np.concatenate([np.arange(s, e + 1, dtype=np.int64) for s, e in KEPT]))      # (8 000 and 20 000 are in two intervals)
    assert covered == int(Targets.contains(job.table[0], job.table[1], kept_positions).sum())
    assert stats["target_intervals_dropped"] == len(DROPPED) and stats["coverage_overflows"] == 0


def test_call_variant_with_region_bed(job, expected, tmp_path, monkeypatch):
    without, _ = _call_variant(monkeypatch, job, str(tmp_path / "plain"), coverage=False, bed=True, fused_inference=True, device_selection=True)
    vcfs, stats = _call_variant(monkeypatch, job, str(tmp_path / "cov"), coverage=True, bed=True, fused_inference=True, device_selection=True)
    assert _read_bed(str(tmp_path / "cov")) == expected[1]
    for name in VCFS:
        assert vcfs[name] == without[name], name
    assert stats["coverage_overflows"] == 0 and stats["coverage_calls"] == stats["encoder_calls"]
