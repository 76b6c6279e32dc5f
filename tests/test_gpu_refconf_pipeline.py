"""options.gvcf through call_variant: PEPPER_VARIANT_FULL.g.vcf.gz beside the five VCFs.

The job of tests/test_gpu_coverage_pipeline.py: a 40 kb contig at ~45x in intervals of 4 kb with two holes in the reads, one of
them a whole interval's fetch range.  What is held here: the five VCFs do not notice the switch; the gVCF's record lines are
the FULL file's; blocks and records tile what the run looked at -- every position lies in exactly one block or under a
record's REF span (records of the FULL file may overlap each other: a deletion over a SNP; no block overlaps any of them);
the file does not depend on threads or encoder_batch; with region_bed no block lies outside a target.  The blocks' values are
held against the numpy rule through the C ABI in tests/test_gpu_refconf.py; here the depth of a block is checked where it is
known without a walk: the holes have MIN_DP 0 and no genotype."""
import gzip
import os

import numpy as np
import pytest

from pepper_amd.variant import Gvcf, Targets, bgzf
from test_gpu_coverage_pipeline import FORMS, HOLES, LENGTH, _call_variant, build_job
from test_gpu_device_sampling import VCFS
from test_gpu_region_bed_pipeline import KEPT

pytestmark = pytest.mark.gpu

MY_FORMS = ["three_step", "fused_device_selection"]
CONFIGS = [(1, 16), (3, 2)]                          # (threads, encoder_batch)


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    return build_job(tmp_path_factory.mktemp("gvcf_job"))


def _run(job, out, gvcf, form, threads=3, bed=False, **over):
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("PEPPER_AMD_GVCF", raising=False)
        extra = dict(gvcf=True) if gvcf else {}
        vcfs, stats = _call_variant(mp, job, out, coverage=False, threads=threads, bed=bed, **FORMS[form], **extra, **over)
    path = os.path.join(out, Gvcf.GVCF_NAME)
    lines = None
    if os.path.exists(path):
        with gzip.open(path, "rb") as fh:
            lines = fh.read().decode().splitlines()
    return vcfs, stats, lines


@pytest.fixture(scope="module")
def plain(job, tmp_path_factory):
    made = {}
    for form in MY_FORMS:
        made[form], stats, lines = _run(job, str(tmp_path_factory.mktemp("gvcf_plain_" + form)), False, form)
        assert lines is None and not any(key.startswith("gvcf") for key in stats)
        assert sum(1 for line in made[form]["PEPPER_VARIANT_FULL"] if not line.startswith("#")) >= 20
    return made


@pytest.fixture(scope="module")
def runs(job, tmp_path_factory):
    made = {}
    for form in MY_FORMS:
        for threads, batch in CONFIGS:
            out = str(tmp_path_factory.mktemp("gvcf_%s_%d" % (form, threads)))
            made[form, threads] = _run(job, out, True, form, threads=threads, encoder_batch=batch) + (out,)
    return made


def _parse(lines):
    """-> (header lines, [(pos0, end0, line)] of the records, [(start0, end0, genotype, gq, min_dp)] of the blocks)."""
    header = [line for line in lines if line.startswith("#")]
    records, blocks = [], []
    for line in lines:
        if line.startswith("#"):
            continue
        f = line.split("\t")
        if f[4] == "<NON_REF>":
            assert f[0] == "ctg" and f[2] == "." and len(f[3]) == 1 and f[5] == "." and f[6] == "." and f[8] == "GT:GQ:MIN_DP", line
            assert f[7].startswith("END=")
            gt, gq, dp = f[9].split(":")
            blocks.append((int(f[1]) - 1, int(f[7][4:]), gt, int(gq), int(dp)))
        else:
            records.append((int(f[1]) - 1, int(f[1]) - 1 + len(f[3]), line))
    return header, records, blocks


def _cover(records, blocks, length=LENGTH):
    in_block, in_record = np.zeros(length, np.int64), np.zeros(length, np.int64)
    for s, e, *_ in blocks:
        in_block[s:e] += 1
    for s, e, _line in records:
        in_record[s:e] += 1
    return in_block, in_record


@pytest.mark.parametrize("threads", [c[0] for c in CONFIGS])
@pytest.mark.parametrize("form", MY_FORMS)
def test_records_blocks_and_tiling(job, plain, runs, form, threads):
    vcfs, stats, lines, out = runs[form, threads]
    for name in VCFS:
        assert vcfs[name] == plain[form][name], name
    header, records, blocks = _parse(lines)
    full = vcfs["PEPPER_VARIANT_FULL"]
    assert [line for _s, _e, line in records] == [line for line in full if not line.startswith("#")]
    full_header = [line for line in full if line.startswith("#")]
    assert header[-1] == full_header[-1] and header[:len(full_header) - 1] == full_header[:-1]
    assert header[len(full_header) - 1:-1] == Gvcf.EXTRA_HEADER.splitlines()
    # sorted, and the tiling: every position the run looked at (the whole contig) in exactly one block, or under a record
    starts = [int(line.split("\t")[1]) for line in lines if not line.startswith("#")]
    assert starts == sorted(starts) and len(blocks) > 50
    in_block, in_record = _cover(records, blocks)
    assert in_block.max() == 1 and ((in_block == 1) != (in_record >= 1)).all()
    # the holes in the reads: no depth, no genotype; elsewhere there are confident blocks
    for lo, hi in HOLES:
        inside = [b for b in blocks if b[0] < hi and b[1] > lo]
        assert inside and all(b[4] == 0 and b[3] == 0 and b[2] == "./." for b in inside if b[0] >= lo and b[1] <= hi)
    assert any(b[2] == "0/0" and b[3] >= 40 and b[4] >= 17 for b in blocks)
    assert all((b[2] == "./.") == (b[4] == 0) for b in blocks)
    # the index is written and names the contig
    assert bgzf.parse_tbi(os.path.join(out, Gvcf.GVCF_NAME + ".tbi"))["names"] == ["ctg"]
    print(form, threads, {k: v for k, v in stats.items() if k.startswith("gvcf") or k == "encoder_calls"})
    # (a first call whose records outgrow the room sized for depth runs is emitted twice and counted: noisy reads change band
    # every few rows; the handle's later calls have the room)
    assert stats["gvcf_overflows"] <= stats["gvcf_calls"] == stats["encoder_calls"] >= threads
    assert stats["gvcf_records"] >= len(blocks) - len(records) - 1 and stats["gvcf_kernel_ms"] > 0.0


def test_the_file_does_not_depend_on_threads_or_encoder_batch(runs):
    for form in MY_FORMS:
        assert runs[form, CONFIGS[0][0]][2] == runs[form, CONFIGS[1][0]][2], form


def test_the_environment_switch(job, runs, tmp_path, monkeypatch):
    out = str(tmp_path / "env")
    with pytest.MonkeyPatch.context() as mp:
        vcfs, _stats = _call_variant(mp, job, out, coverage=False, threads=2)
    assert not os.path.exists(os.path.join(out, Gvcf.GVCF_NAME))
    out = str(tmp_path / "env_on")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PEPPER_AMD_GVCF", "1")
        _call_variant(mp, job, out, coverage=False, threads=2)
    with gzip.open(os.path.join(out, Gvcf.GVCF_NAME), "rb") as fh:
        assert fh.read().decode().splitlines() == runs["three_step", 1][2]


def test_with_region_bed_no_block_outside_a_target(job, tmp_path):
    without, _stats, none = _run(job, str(tmp_path / "plain"), False, "fused_device_selection", bed=True)
    vcfs, stats, lines = _run(job, str(tmp_path / "gvcf"), True, "fused_device_selection", bed=True)
    assert none is None
    for name in VCFS:
        assert vcfs[name] == without[name], name
    _header, records, blocks = _parse(lines)
    in_block, in_record = _cover(records, blocks)
    positions = np.arange(LENGTH, dtype=np.int64)
    on_target = Targets.contains(job.table[0], job.table[1], positions)
    looked_at = np.zeros(LENGTH, bool)
    for s, e in KEPT:
        looked_at[s:e + 1] = True
    assert len(blocks) >= 10 and not in_block[~on_target].any() and not in_block[~looked_at].any()
    want = on_target & looked_at
    assert in_block.max() == 1 and ((in_block[want] == 1) != (in_record[want] >= 1)).all()
    assert stats["gvcf_overflows"] <= stats["gvcf_calls"] == stats["encoder_calls"]
