"""options.region_bed through the image-generation driver and call_variant: the run restricted to a BED against the
unrestricted run of the same form, filtered on the host by Targets.contains.

A 40 kb contig at ~45x in intervals of 4 kb (the job of tests/test_gpu_device_candidates_pipeline.py, with SNPs planted on two
interval boundaries).  The BED leaves three of the ten intervals without a target, has a target of one base on the boundary at
8 000 (which keeps both neighbours, each with that candidate) and cuts through the pile of short reads on 21 - 22 kb.  Image
files: the groups are exactly the kept intervals', each the unrestricted group's rows inside the targets, dataset by dataset.
VCFs: the data lines are the unrestricted run's lines whose POS - 1 is a target, line for line (one contig: a site is a
position, the finder merges per site and the writer's duplicate-start rule compares the starts of consecutive sites)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pileup_utils as pu
from pepper_amd import synthetic
from pepper_amd.variant import Targets
from test_gpu_device_sampling import VCFS, _clean, _variant_groups, _variant_options, _write

pytestmark = pytest.mark.gpu

REGION_SIZE = 4000
# eleven lines, ten intervals after the merge; no target inside 12 000 - 16 000, 24 000 - 28 000 and 32 000 - 36 000
BED_TEXT = ("# targets of the region_bed pipeline test\n"
            "ctg\t500\t1500\nctg\t5000\t5400\nctg\t8000\t8001\nctg\t8900\t9001\nctg\t10500\t11000\n"
            "ctg\t16100\t17000\nctg\t20000\t20050\n\nctg\t21300\t21500\tpile\nctg  21450 21700\n"
            "ctg\t29900\t30100\nctg\t36500\t37500\nunplaced\t0\t1000\n")
KEPT = [(0, 4000), (4000, 8000), (8000, 12000), (16000, 20000), (20000, 24000), (28000, 32000), (36000, 39999)]
DROPPED = [(12000, 16000), (24000, 28000), (32000, 36000)]


def build_job(tmp):
    rng = np.random.default_rng(4021)
    ref = pu.random_reference(rng, 40000, n_frac=0.001)

    def other(p):
        return "ACGT"[(("ACGT".index(ref[p]) if ref[p] in "ACGT" else 0) + 1) % 4]
    sites = {int(p): (other(int(p)), 0.5) for p in rng.choice(np.arange(300, 39500), 260, replace=False)}
    for p in (8000, 20000, 21300, 21699, 21700):           # two interval boundaries inside targets, the edges of the cut through the pile
        sites[p] = (other(p), 0.5)
    indels = {5100: ("I", "ACGTACGTTTGACA", 0.4), 9000: ("D", 12, 0.5), 21400: ("I", "CAG", 0.5), 21600: ("D", 4, 0.5),
              30000: ("I", "TT", 0.6)}
    reads = _clean(pu.simulate_reads(rng, ref, 0, n_reads=1000, read_len=(500, 4000), snp_sites=sites, indel_sites=indels, clip_rate=0.3))
    reads += _clean(pu.simulate_reads(rng, ref[21000:22200], 21000, n_reads=700, read_len=(200, 500), snp_sites=sites, indel_sites=indels))
    bam, fa = _write(tmp, [("ctg", ref)], reads)
    sd = synthetic.variant_state_dict(seed=96, gain=2.5)
    model = str(tmp / "model.pkl")
    torch.save(synthetic.checkpoint_dict({k: torch.from_numpy(v) for k, v in sd.items()}, hidden_size=128), model)
    bed = str(tmp / "targets.bed")
    with open(bed, "w") as fh:
        fh.write(BED_TEXT)
    table = Targets.read_bed(bed, {"ctg": len(ref)})["ctg"]
    assert len(table[0]) == 10
    return SimpleNamespace(bam=bam, fasta=fa, model=model, bed=bed, table=table)


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    return build_job(tmp_path_factory.mktemp("region_bed_job"))


def _name(s, e):
    return "ctg_%d_%d" % (s, e)


def _inside(job, positions):
    return Targets.contains(job.table[0], job.table[1], positions)


def _filtered_group(job, group):
    keep = _inside(job, group["positions"])
    return {key: ([v for v, k in zip(value, keep) if k] if isinstance(value, list) else value[keep]) for key, value in group.items()}


def _generate(monkeypatch, job, out, bed, threads=1, packed=True, device_candidates=False, **over):
    from pepper_amd.variant.ImageGenerationUI import ImageGenerationUtils
    monkeypatch.setenv("PEPPER_AMD_PACKED_READS", "1" if packed else "0")
    monkeypatch.setenv("PEPPER_AMD_DEVICE_CANDIDATES", "1" if device_candidates else "0")
    stats = {}
    options = _variant_options(job.bam, job.fasta, out, region_size=REGION_SIZE, threads=threads, stage_seconds=stats, **over)
    if bed:
        options.region_bed = job.bed                   # (off: the attribute does not exist, as in every other test's options)
    ImageGenerationUtils.generate_images(options)
    return _variant_groups(out), stats


@pytest.fixture(scope="module")
def unrestricted(job, tmp_path_factory):
    """The yardstick of the image files: the packed form's unrestricted run (tests/test_gpu_packed.py holds the host-clipped form
    to it, tests/test_gpu_device_candidates_pipeline.py the device enumeration), and that the comparison is not vacuous."""
    with pytest.MonkeyPatch.context() as mp:
        groups, stats = _generate(mp, job, str(tmp_path_factory.mktemp("region_bed_full")), bed=False)
    assert stats["target_calls"] == 0 and "target_intervals_dropped" not in stats
    assert sorted(groups) == sorted(_name(s, e) for s, e in KEPT + DROPPED)
    positions = np.concatenate([g["positions"] for g in groups.values()])
    inside = _inside(job, positions)
    print("unrestricted: %d candidates, %d inside the targets, %d outside" % (len(positions), inside.sum(), (~inside).sum()))
    assert len(positions) > 150 and inside.sum() >= 30 and (~inside).sum() >= 30
    # the candidate on the shared boundary at 8 000 is in both neighbours' groups
    assert 8000 in groups[_name(4000, 8000)]["positions"] and 8000 in groups[_name(8000, 12000)]["positions"]
    assert all(len(groups[_name(s, e)]["positions"]) > 0 for s, e in DROPPED)
    return groups


def _check_groups(job, got, want_full, kept=KEPT):
    assert sorted(got) == sorted(_name(s, e) for s, e in kept)          # dropped intervals have no group
    n = 0
    for name in got:
        want = _filtered_group(job, want_full[name])
        for key in want:
            x, y = got[name][key], want[key]
            assert (x == y) if isinstance(x, list) else (x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)), (name, key)
        n += len(want["candidates"])
    return n


@pytest.mark.parametrize("threads,packed,device_candidates", [(1, True, False), (3, True, False), (1, False, False), (3, False, False),
                                                              (1, True, True), (3, True, True)])
def test_image_files_are_the_unrestricted_ones_filtered(job, unrestricted, tmp_path, monkeypatch, threads, packed, device_candidates):
    got, stats = _generate(monkeypatch, job, str(tmp_path / "bed"), bed=True, threads=threads, packed=packed,
                           device_candidates=device_candidates)
    print({k: stats.get(k) for k in ("target_intervals_dropped", "target_calls", "encoder_calls", "host_form_intervals",
                                     "device_enumerated_calls", "host_enumerated_calls")})
    assert _check_groups(job, got, unrestricted) >= 30
    assert 8000 in got[_name(4000, 8000)]["positions"] and 8000 in got[_name(8000, 12000)]["positions"]
    assert stats["target_intervals_dropped"] == len(DROPPED)
    if packed:
        # every encoder call of every worker ran with its contig's table set
        assert stats["target_calls"] == stats["encoder_calls"] >= threads and stats.get("host_form_intervals", 0) == 0
        assert stats["device_enumerated_calls"] == (stats["encoder_calls"] if device_candidates else 0)
        assert stats["host_enumerated_calls"] == 0
    else:
        # the host-clipped form: one call per worker (its intervals are one group of one contig)
        assert stats["target_calls"] == threads and stats["host_form_intervals"] == len(KEPT) and stats["encoder_calls"] == 0


def test_region_and_bed_intersect(job, tmp_path, monkeypatch):
    full, _ = _generate(monkeypatch, job, str(tmp_path / "full"), bed=False, region="ctg:8000-30000")
    got, stats = _generate(monkeypatch, job, str(tmp_path / "bed"), bed=True, region="ctg:8000-30000")
    kept = [(8000, 12000), (16000, 20000), (20000, 24000), (28000, 30000)]
    assert sorted(full) == sorted(_name(s, e) for s, e in kept + [(12000, 16000), (24000, 28000)])
    assert _check_groups(job, got, full, kept) >= 15 and stats["target_intervals_dropped"] == 2


def test_a_bed_run_then_an_unrestricted_run_in_one_process(job, unrestricted, tmp_path, monkeypatch):
    """One worker, so the second run's worker takes the handle the first one's worker returned to the pool -- and this
    thread's handle serves both host-clipped runs."""
    from test_gpu_device_sampling import _same_groups
    for packed in (True, False):
        tag = "packed" if packed else "host"
        got, _ = _generate(monkeypatch, job, str(tmp_path / (tag + "_bed")), bed=True, packed=packed)
        assert _check_groups(job, got, unrestricted) >= 30
        after, stats = _generate(monkeypatch, job, str(tmp_path / (tag + "_after")), bed=False, packed=packed)
        assert _same_groups(after, unrestricted) > 150 and stats["target_calls"] == 0


def _call_variant(monkeypatch, job, out, bed, **over):
    from pepper_amd.variant.CallVariant import call_variant
    monkeypatch.setenv("PEPPER_AMD_BATCH_INVARIANT", "1")
    monkeypatch.setenv("PEPPER_AMD_PACKED_READS", "1")
    monkeypatch.setenv("PEPPER_AMD_DEVICE_CANDIDATES", "0")
    monkeypatch.delenv("PEPPER_AMD_DEVICE_SELECTION", raising=False)
    monkeypatch.delenv("PEPPER_AMD_FUSED_CALL_VARIANT", raising=False)
    stats = {}
    o = _variant_options(
        job.bam, job.fasta, None, region=None, region_size=REGION_SIZE, threads=3, output_dir=out,
        model_path=job.model, batch_size=128, num_workers=0, gpu=True, device_ids="0", callers_per_gpu=1,
        quantized=False, dry=False, sample_name="SYN", allowed_multiallelics=4,
        snp_p_value=0.1, insert_p_value=0.25, delete_p_value=0.25, snp_p_value_in_lc=0.1,
        insert_p_value_in_lc=0.3, delete_p_value_in_lc=0.3, snp_q_cutoff=20, indel_q_cutoff=15,
        snp_q_cutoff_in_lc=20, indel_q_cutoff_in_lc=10, report_snp_above_freq=0, report_indel_above_freq=0,
        stage_seconds=stats, **over)
    del o.image_output_directory
    if bed:
        o.region_bed = job.bed
    _, o.prediction_directory, _ = call_variant(o)
    stats["options"] = o
    return _vcfs(out), stats


def _vcfs(out):
    from pepper_amd.variant import bgzf
    return {name: bgzf.read_bgzf(os.path.join(out, name + ".vcf.gz")).decode().splitlines() for name in VCFS}


@pytest.mark.parametrize("form", ["three_step", "fused", "fused_device_selection"])
def test_call_variant_vcfs_are_the_unrestricted_ones_filtered(job, tmp_path, monkeypatch, form):
    over = {"three_step": {}, "fused": dict(fused_inference=True),
            "fused_device_selection": dict(fused_inference=True, device_selection=True)}[form]
    want, _ = _call_variant(monkeypatch, job, str(tmp_path / "full"), bed=False, **over)
    got, stats = _call_variant(monkeypatch, job, str(tmp_path / "bed"), bed=True, **over)
    assert stats["target_intervals_dropped"] == len(DROPPED) and stats["target_calls"] == stats["encoder_calls"] >= 3
    kept_lines = 0
    for name in VCFS:
        head = [line for line in want[name] if line.startswith("#")]
        data = [line for line in want[name] if not line.startswith("#")]
        inside = _inside(job, np.array([int(line.split("\t")[1]) - 1 for line in data], np.int64))
        expected = head + [line for line, k in zip(data, inside) if k]
        if name == "PEPPER_VARIANT_FULL":
            print(form, "full VCF: %d records, %d inside the targets" % (len(data), inside.sum()))
            assert inside.sum() >= 20 and (~inside).sum() >= 20
        assert len(got[name]) == len(expected), name
        for g, w in zip(got[name], expected):
            assert g == w, (name, g, w)
        kept_lines += int(inside.sum())
    assert kept_lines > 40


def test_the_finder_over_filtered_predictions_gives_the_restricted_vcfs(job, tmp_path, monkeypatch):
    """What the line-for-line expectation above relies on, checked with the host finder itself: the unrestricted three-step
    run's prediction files, cut down to the rows whose position is a target, go through process_candidates -- the five VCFs are
    those of the run with the BED, line for line."""
    from pepper_amd import h5
    from pepper_amd.variant.DataStorePredict import DataStore
    from pepper_amd.variant.FindCandidates import get_file_paths_from_directory, process_candidates
    _, full = _call_variant(monkeypatch, job, str(tmp_path / "full"), bed=False)
    got, _ = _call_variant(monkeypatch, job, str(tmp_path / "bed"), bed=True)
    filtered = tmp_path / "filtered_predictions"
    filtered.mkdir()
    rows = kept = 0
    for path in get_file_paths_from_directory(full["options"].prediction_directory):
        with h5.File(path) as f, DataStore(str(filtered / os.path.basename(path)), "w") as store:
            for k, key in enumerate(f.keys("predictions")):
                g = "predictions/" + key + "/"
                positions = np.asarray(f[g + "positions"])
                keep = _inside(job, positions)
                rows, kept = rows + len(keep), kept + int(keep.sum())
                if keep.any():
                    store.write_prediction(k, np.asarray(f[g + "contigs"])[keep], positions[keep], np.asarray(f[g + "depths"])[keep],
                                           np.asarray(f[g + "candidates"], dtype=object)[keep],
                                           np.asarray(f[g + "candidate_frequency"])[keep], np.asarray(f[g + "base_prediction"])[keep])
    print("prediction rows: %d, %d inside the targets" % (rows, kept))
    assert kept >= 30 and rows - kept >= 30
    out = str(tmp_path / "from_filtered")
    process_candidates(full["options"], str(filtered), out)
    want = _vcfs(out)
    for name in VCFS:
        assert len(got[name]) == len(want[name]), name
        for g, w in zip(got[name], want[name]):
            assert g == w, (name, g, w)
    assert sum(1 for line in want["PEPPER_VARIANT_FULL"] if not line.startswith("#")) >= 20
