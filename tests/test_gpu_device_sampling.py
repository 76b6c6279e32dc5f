"""The reservoir sample of deep intervals drawn on the device (reservoir_keep_kernel, pa_encoder_set_sampling) against the host
forms, which draw it with numpy.random.RandomState as the reference does: image files of both pipelines equal dataset by dataset,
the fused callers' outputs identical, and at the handle the kept pairs equal to pa_reservoir_sample's slots.  The host side of
every comparison is the same run under PEPPER_AMD_DEVICE_SAMPLING=0 (the routing before the kernel existed), which
tests/test_gpu_packed.py, test_gpu_polish_chain.py and test_gpu_images_vs_ref.py hold to the reference's own builds."""
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bam_utils as bu
import pileup_utils as pu
from pepper_amd import h5, synthetic

pytestmark = pytest.mark.gpu

SEED = 2719747673
VARIANT_CAP, POLISH_CAP = 5000, 1500


def _clean(reads):
    return [r for r in reads if not any(op in (3, 6) for op, _ in r["cigar"])]


def _write(tmp, refs, reads, name="in"):
    bam, fa = str(tmp / (name + ".bam")), str(tmp / (name + ".fa"))
    reads = sorted(reads, key=lambda r: r["pos"])
    for i, r in enumerate(reads):
        r["name"] = "q%d" % i
    bu.write_bam(bam, [(n, len(s)) for n, s in refs], {0: reads}, flush_every=47)
    with open(fa, "w") as fh:
        for n, s in refs:
            fh.write(">" + n + "\n" + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    return bam, fa


# ---- variant ---------------------------------------------------------------------------------------------------------------
def _variant_options(bam, fasta, out, **over):
    o = SimpleNamespace(
        bam=bam, fasta=fasta, region="ctg", region_size=2000, threads=2, train_mode=False, use_hp_info=False,
        image_output_directory=out, include_supplementary=False, min_mapq=1, min_snp_baseq=1, min_indel_baseq=1,
        snp_frequency=0.10, insert_frequency=0.15, delete_frequency=0.15, min_coverage_threshold=3,
        snp_candidate_frequency_threshold=0.10, indel_candidate_frequency_threshold=0.12, candidate_support_threshold=2,
        skip_indels=False, downsample_rate=1.0)
    for k, v in over.items():
        setattr(o, k, v)
    return o


def _variant_groups(directory):
    out = {}
    for fn in sorted(os.listdir(directory)):
        with h5.File(os.path.join(directory, fn)) as f:
            for name in (f.keys("summaries") if "summaries" in f else []):
                assert name not in out
                g = "summaries/" + name + "/"
                out[name] = dict(images=f[g + "images"], positions=f[g + "positions"], depths=f[g + "depths"],
                                 candidates=f[g + "candidates"].tolist(), freq=f[g + "candidate_frequency"], contigs=f[g + "contigs"].tolist())
    return out


def _same_groups(a, b):
    assert sorted(a) == sorted(b)
    n = 0
    for name in a:
        for key in a[name]:
            x, y = a[name][key], b[name][key]
            assert (x == y) if isinstance(x, list) else (x.dtype == y.dtype and np.array_equal(x, y)), (name, key)
        n += len(a[name]["candidates"])
    return n


@pytest.fixture(scope="module")
def deep_job(tmp_path_factory):
    """A 12 kb contig in intervals of 2 kb (fetched +- 100): an ordinary stretch; a pile of ~5 600 short reads (6 400 drawn, mapq 0 and skips dropped) inside the
    interval 4 000 - 6 000; a second pile on 7 300 - 8 150 of 4 700 reads that reach over the boundary at 8 000 and 500 that
    end in front of it with a deletion whose bases alone reach into the next interval's fetch range (7 900 ...): more than
    5 000 (read, interval) pairs for BOTH neighbours, more than 5 000 reads in the left one, fewer in the right one."""
    tmp = tmp_path_factory.mktemp("deep_job")
    rng = np.random.default_rng(2025)
    ref = pu.random_reference(rng, 12000)
    sites = {int(p): ("ACGT"[("ACGT".index(ref[p]) + 1) % 4], 0.5) for p in rng.choice(np.arange(200, 11800), 70, replace=False)}
    indels = {4800: ("I", "CAG", 0.5), 5200: ("D", 4, 0.6), 1500: ("I", "TT", 0.6), 7400: ("D", 3, 0.5)}
    reads = _clean(pu.simulate_reads(rng, ref, 0, n_reads=420, read_len=(400, 2500), snp_sites=sites, indel_sites=indels))
    reads += _clean(pu.simulate_reads(rng, ref[4300:5700], 4300, n_reads=6400, read_len=(150, 300), snp_sites=sites, indel_sites=indels))

    def plain(pos, n, tail_deletion=0):
        seq = list(ref[pos:pos + n])
        for p, (alt, frac) in sites.items():
            if pos <= p < pos + n and rng.random() < frac:
                seq[p - pos] = alt
        for k in np.flatnonzero(rng.random(n) < 0.02):
            seq[k] = "ACGT"[int(rng.integers(0, 4))]
        cigar = [(0, n)] + ([(2, tail_deletion)] if tail_deletion else [])
        return dict(pos=int(pos), reverse=bool(rng.random() < 0.5), mapq=60, seq="".join(seq),
                    qual=rng.integers(5, 40, n).astype(np.uint8), cigar=cigar)
    for _ in range(4700):                      # a base on both sides of 8 000
        pos = int(rng.integers(7700, 7890))
        reads.append(plain(pos, int(rng.integers(7920 - pos, 8150 - pos))))
    for _ in range(500):                       # last base at 7 899 or before; the trailing deletion covers 7 900 and more
        pos = int(rng.integers(7300, 7750))
        n = int(rng.integers(100, 7890 - pos))
        reads.append(plain(pos, n, tail_deletion=7910 - (pos + n) + int(rng.integers(0, 20))))
    bam, fa = _write(tmp, [("ctg", ref)], reads)
    sd = synthetic.variant_state_dict(seed=95, gain=2.5)
    model = str(tmp / "model.pkl")
    torch.save(synthetic.checkpoint_dict({k: torch.from_numpy(v) for k, v in sd.items()}, hidden_size=128), model)
    return SimpleNamespace(bam=bam, fasta=fa, model=model, ref=ref)


def _generate(monkeypatch, job, out, device_sampling, **over):
    from pepper_amd.variant.ImageGenerationUI import ImageGenerationUtils
    monkeypatch.setenv("PEPPER_AMD_DEVICE_SAMPLING", "1" if device_sampling else "0")
    stats = {}
    ImageGenerationUtils.generate_images(_variant_options(job.bam, job.fasta, out, stage_seconds=stats, **over))
    return _variant_groups(out), stats


def test_the_job_has_the_piles_it_claims(deep_job):
    """Per interval: (read, interval) pairs of the packer against reads with a base inside (get_reads)."""
    from pepper_amd.variant.bam import BAM_handler
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    handler = BAM_handler(deep_job.bam)
    starts = [max(0, a - 100) for a in range(0, 12000, 2000)]
    stops = [min(11999, a + 2000) + 100 for a in range(0, 12000, 2000)]
    enc = PackedEncoder(0, arena_bytes=64 << 20)
    n_done, region_pairs, _counts = enc.pack(handler, "ctg", starts, stops, False, 1)
    enc.close()
    assert n_done == 6
    pairs = np.diff(region_pairs[:7])
    live = [len(handler.get_reads("ctg", a, b, False, 1, 1)) for a, b in zip(starts, stops)]
    print("pairs", pairs.tolist(), "reads", live)
    assert pairs[2] > VARIANT_CAP and live[2] > VARIANT_CAP                      # the pile inside 4 000 - 6 000
    assert pairs[3] > VARIANT_CAP and live[3] > VARIANT_CAP                      # left of the boundary: sampled
    assert pairs[4] > VARIANT_CAP and 0 < live[4] <= VARIANT_CAP                 # right of it: pairs beyond the cap, reads not
    assert 0 < live[0] < VARIANT_CAP and 0 < live[5] < VARIANT_CAP


def test_variant_image_files_equal_the_host_form(deep_job, tmp_path, monkeypatch):
    got, stats = _generate(monkeypatch, deep_job, str(tmp_path / "device"), True)
    want, stats_host = _generate(monkeypatch, deep_job, str(tmp_path / "host"), False)
    print("device", {k: stats.get(k) for k in ("sampled_on_device", "host_form_intervals")},
          "host", {k: stats_host.get(k) for k in ("sampled_on_device", "host_form_intervals")})
    assert _same_groups(got, want) > 40
    assert stats["sampled_on_device"] > 0 and stats.get("host_form_intervals", 0) == 0
    assert stats_host["sampled_on_device"] == 0 and stats_host["host_form_intervals"] > 0
    assert any(name.startswith("ctg_4000_") for name in got) and any(name.startswith("ctg_8000_") for name in got)


def test_variant_downsample_rate_stays_on_the_device(deep_job, tmp_path, monkeypatch):
    got, stats = _generate(monkeypatch, deep_job, str(tmp_path / "device"), True, downsample_rate=0.5)
    want, stats_host = _generate(monkeypatch, deep_job, str(tmp_path / "host"), False, downsample_rate=0.5)
    assert _same_groups(got, want) > 20
    assert stats["sampled_on_device"] >= len(got) and stats.get("host_form_intervals", 0) == 0 and "encode" in stats
    assert stats_host["host_form_intervals"] >= len(want) and "encode" not in stats_host
    full, _ = _generate(monkeypatch, deep_job, str(tmp_path / "full"), True)
    assert any(not np.array_equal(full[name]["depths"], got[name]["depths"]) for name in got if name in full)   # (half the reads)


def test_handle_keeps_the_slots_of_the_host_sampler(deep_job):
    """PackedEncoder.encode(..., sampling=...) on the interval 4 000 - 6 000 alone."""
    from pepper_amd import _lib
    from pepper_amd.variant.bam import BAM_handler
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    params = (1, 1, 0.1, 0.15, 0.15, 3, 0.1, 0.12, 2, False)
    handler = BAM_handler(deep_job.bam)
    enc = PackedEncoder(0, arena_bytes=64 << 20)

    def encode(a, b, sampling):
        lo, hi = max(0, a - 100), b + 100
        n_done, region_pairs, counts = enc.pack(handler, "ctg", [lo], [hi], False, 1)
        assert n_done == 1
        outs, live = enc.encode([(lo, hi)], [deep_job.ref[lo:hi + 1]], region_pairs, counts, params, [(a, b)], sampling=sampling)
        return outs[0], int(live[0]), enc.pair_live(int(region_pairs[1]))
    plain, n, live_pairs = encode(4000, 6000, None)
    assert n > VARIANT_CAP and int(live_pairs.sum()) == n and enc.sampled() == (0, 0)
    ranks = np.flatnonzero(live_pairs)                    # rank among the interval's reads -> pair
    sampled_regions = dropped = 0
    for rate in (1.0, 0.5, 0.999):
        k = int(min(VARIANT_CAP, rate * n))
        out, kept, keep = encode(4000, 6000, (SEED, VARIANT_CAP, rate))
        assert kept == k
        assert np.flatnonzero(keep).tolist() == sorted(ranks[_lib.reservoir_sample(SEED, n, k)].tolist())
        sampled_regions, dropped = sampled_regions + 1, dropped + n - k
        assert enc.sampled() == (sampled_regions, dropped)
        assert len(out["positions"]) > 0
    # an empty sample: int(0.0001 * n) == 0 clears the interval
    out, kept, keep = encode(4000, 6000, (SEED, VARIANT_CAP, 0.0001))
    assert kept == 0 and not keep.any() and len(out["positions"]) == 0
    assert enc.sampled() == (sampled_regions + 1, dropped + n)
    # sampling set and nothing to sample: outputs and counters as without it
    before = enc.sampled()
    want, n0, pairs0 = encode(0, 2000, None)
    got, n1, pairs1 = encode(0, 2000, (SEED, VARIANT_CAP, 1.0))
    assert 0 < n0 == n1 < VARIANT_CAP and np.array_equal(pairs0, pairs1) and enc.sampled() == before
    assert sorted(got) == sorted(want) and len(want["positions"]) > 0
    for key in want:
        assert (got[key] == want[key]) if isinstance(want[key], list) else np.array_equal(got[key], want[key]), key
    # off again: the deep interval as the first call saw it
    again, n2, pairs2 = encode(4000, 6000, None)
    assert n2 == n and np.array_equal(pairs2, live_pairs) and np.array_equal(again["images"], plain["images"])
    with pytest.raises(_lib.PepperAmdError):
        enc.set_sampling((SEED, 5001, 1.0))
    enc.close()


VCFS = ("PEPPER_VARIANT_FULL", "PEPPER_VARIANT_OUTPUT_PEPPER", "PEPPER_VARIANT_OUTPUT_VARIANT_CALLING",
        "PEPPER_VARIANT_OUTPUT_VARIANT_CALLING_SNPs", "PEPPER_VARIANT_OUTPUT_VARIANT_CALLING_INDEL")


def test_fused_call_variant_vcfs_identical_to_the_host_sampled_run(deep_job, tmp_path, monkeypatch):
    from pepper_amd.variant import bgzf
    from pepper_amd.variant.CallVariant import call_variant
    monkeypatch.setenv("PEPPER_AMD_BATCH_INVARIANT", "1")

    def run(out, device_sampling):
        monkeypatch.setenv("PEPPER_AMD_DEVICE_SAMPLING", "1" if device_sampling else "0")
        o = _variant_options(
            deep_job.bam, deep_job.fasta, None, region=None, threads=3, output_dir=out, fused_inference=True,
            model_path=deep_job.model, batch_size=128, num_workers=0, gpu=True, device_ids="0", callers_per_gpu=1,
            quantized=False, dry=False, sample_name="SYN", allowed_multiallelics=4,
            snp_p_value=0.1, insert_p_value=0.25, delete_p_value=0.25, snp_p_value_in_lc=0.1,
            insert_p_value_in_lc=0.3, delete_p_value_in_lc=0.3, snp_q_cutoff=20, indel_q_cutoff=15,
            snp_q_cutoff_in_lc=20, indel_q_cutoff_in_lc=10, report_snp_above_freq=0, report_indel_above_freq=0)
        del o.image_output_directory
        _, _, totals = call_variant(o)
        return totals, {name: bgzf.read_bgzf(os.path.join(out, name + ".vcf.gz")).decode().splitlines() for name in VCFS}
    totals, got = run(str(tmp_path / "device"), True)
    totals_host, want = run(str(tmp_path / "host"), False)
    assert totals == totals_host and totals[0] > 30
    for name in VCFS:
        assert len(got[name]) == len(want[name]), name
        for g, w in zip(got[name], want[name]):
            assert g == w, (name, g, w)


# ---- polish ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def polish_job(tmp_path_factory):
    """A 9.4 kb draft with a pile of short reads on 5 100 - 5 500, as tests/test_gpu_polish_chain.py's deep dataset (more reads
    drawn: simulate_reads' skips are dropped, which leaves ~1 800 of the pile's 2 300 and ~80 of the 900 ordinary ones)."""
    tmp = tmp_path_factory.mktemp("polish_job")
    rng = np.random.default_rng(98)
    draft = pu.random_reference(rng, 9400)
    reads = _clean(pu.simulate_reads(rng, draft, 0, n_reads=900, read_len=(400, 2600), ins_rate=0.03, del_rate=0.03))
    reads += _clean(pu.simulate_reads(rng, draft[5100:5500], 5100, n_reads=2300, read_len=(120, 260), ins_rate=0.02, del_rate=0.02))
    bam, fa = _write(tmp, [("ctg1", draft)], reads, name="polish")
    with open(fa, "w") as fh:
        fh.write(">ctg1\n" + draft + "\n")
    psd = synthetic.polish_state_dict(seed=19, gain=2.0)
    model = str(tmp / "polish.pkl")
    torch.save(synthetic.checkpoint_dict({k: torch.from_numpy(v) for k, v in psd.items()}, hidden_size=128), model)
    return SimpleNamespace(bam=bam, fasta=fa, model=model)


def _polish_groups(out_dir):
    merged = {}
    for path in glob.glob(os.path.join(out_dir, "*.hdf")):
        with h5.File(path) as f:
            for name in f.keys("summaries"):
                base = "summaries/" + name + "/"
                assert name not in merged
                merged[name] = {k: np.asarray(f[base + k]) for k in ("image", "label", "position", "index", "region_start", "region_end", "chunk_id")}
                merged[name]["contig"] = f[base + "contig"]
    return merged


def _make_images(monkeypatch, job, out_dir, threads, chain=True, device_sampling=True, regions=None, **kw):
    from pepper_amd.polish import ImageGenerationUI as ui
    from pepper_amd.polish.make_images import make_images
    monkeypatch.setenv("PEPPER_AMD_POLISH_CHAIN", "1" if chain else "0")
    monkeypatch.setenv("PEPPER_AMD_DEVICE_SAMPLING", "1" if device_sampling else "0")
    if regions is not None:
        monkeypatch.setattr(ui.UserInterfaceSupport, "CHAIN_REGIONS", regions)
    stats = {}
    make_images(job.bam, job.fasta, None, out_dir, threads, stats=stats, **kw)
    return _polish_groups(out_dir), stats


def _assert_same_polish(got, want):
    assert sorted(got) == sorted(want)
    for name in want:
        for key, w in want[name].items():
            g = got[name][key]
            assert (g == w) if isinstance(w, (str, bytes)) else np.array_equal(g, w), (name, key)


@pytest.mark.parametrize("threads,regions", [(1, 128), (3, 2)])
def test_polish_chain_files_equal_the_host_form(polish_job, tmp_path, monkeypatch, threads, regions):
    want, _ = _make_images(monkeypatch, polish_job, str(tmp_path / "host"), 1, chain=False)
    got, stats = _make_images(monkeypatch, polish_job, str(tmp_path / "chain"), threads, regions=regions)
    print({k: stats.get(k) for k in ("sampled_on_device", "host_form_intervals")})
    assert any(name.startswith("ctg1_4900_") for name in want) and len(want) >= 10
    _assert_same_polish(got, want)
    assert stats["sampled_on_device"] > 0 and stats.get("host_form_intervals", 0) == 0 and "chain" in stats
    # ... and the earlier routing: the deep intervals blanked out of the chain call and redone by the host form
    old, stats_old = _make_images(monkeypatch, polish_job, str(tmp_path / "old"), threads, device_sampling=False, regions=regions)
    _assert_same_polish(old, want)
    assert stats_old["sampled_on_device"] == 0 and stats_old["host_form_intervals"] > 0


def test_polish_downsample_rate_goes_through_the_chain(polish_job, tmp_path, monkeypatch):
    want, _ = _make_images(monkeypatch, polish_job, str(tmp_path / "one"), 2)
    got, stats = _make_images(monkeypatch, polish_job, str(tmp_path / "half"), 2, downsample_rate=0.5)
    _assert_same_polish(got, want)
    assert "chain" in stats and stats["sampled_on_device"] > 0 and stats.get("host_form_intervals", 0) == 0


def test_fused_polish_with_a_downsample_rate(polish_job, tmp_path, monkeypatch):
    from pepper_amd.polish.polish import polish
    monkeypatch.setenv("PEPPER_AMD_POLISH_CHAIN", "1")
    monkeypatch.setenv("PEPPER_AMD_DEVICE_SAMPLING", "1")
    texts = {}
    for name, kw in (("three_step", dict(fused_inference=False)), ("fused", dict(fused_inference=True, downsample_rate=0.5))):
        out_dir = str(tmp_path / name) + "/"
        polish(polish_job.bam, polish_job.fasta, out_dir, 2, None, polish_job.model, 64, True, "0", 0, **kw)
        fasta = glob.glob(out_dir + "*.fa")
        assert len(fasta) == 1
        texts[name] = open(fasta[0]).read()
    assert texts["three_step"].startswith(">ctg1") and len(texts["three_step"]) > 9000
    assert texts["fused"] == texts["three_step"]
