"""Stitch rate (prediction HDF5 files -> polished FASTA): perform_stitch with the merge inside the I/O library (default) and with
the numpy form (PEPPER_AMD_STITCH_NUMPY=1), one and eight workers; --device adds the same set through the device stitch
(pepper_amd/polish/DeviceStitch.py stitch_directory: the files read on the host, the merge on the GPU) and checks its FASTA
against the host's.  --qualities runs the set with qualities on as well -- perform_stitch(..., qualities=True) on the host (the
numpy merge with a phred column) and, with --device, stitch_directory(..., qualities=True) -- and checks the two FASTQ files equal.
--edits runs the set with the edits on as well, against a seeded random draft (the labels are random too, so four slots in five
are an edit: the record buffer's worst case, not a polished assembly's share) -- perform_stitch(..., edits=draft) on the host and,
with --device, stitch_directory(..., edits=draft) -- and checks the two .edits.tsv files equal.
--fill runs the set with fill on as well, against the same draft (the job's rows cover the draft but for its last 1 200 letters, so
the filling is one trailing run) -- perform_stitch(..., fill=draft) on the host and, with --device, stitch_directory(..., fill=draft),
checked against the host's FASTA -- and then, on one handle that holds the job's rows, times finish + take without fill beside
finish + fill + take (one warm-up and three timed calls each; pa_stitcher_fill's own seconds beside them).
--min-quality Q runs the set with the gate on as well, against the same draft (random labels: four slots in five are an edit, and
with phred uniform in 0..100 a share Q / 101 of them is withheld) -- perform_stitch(..., min_quality=Q, draft=draft) on the host
and, with --device, stitch_directory(..., min_quality=Q, draft=draft), FASTA and .withheld.tsv checked against the host's -- and
then, on one handle that holds the job's rows with their phred, times finish + take beside finish + gate + take (+ the withheld
records' copy back), one warm-up and three timed calls each.
--vcf (with --device) holds the job's rows with their phred on one handle, fills once against the same draft, and times three
things on the same edit records, one warm-up and three timed calls each: the edit comparison with its copy back
(pa_stitcher_edits + take), the variant normalisation with its copy back (pa_stitcher_variants + take) and the numpy twin
(Variants.records_numpy); the device's records are checked against the twin's bytes.
    python tools/bench_stitch.py [--chunks 65536] [--files 4] [--dir /dev/shm] [--device] [--qualities] [--edits] [--fill]
                                 [--min-quality Q] [--vcf]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pepper_amd.polish.DataStorePredict import DataStore  # noqa: E402
from pepper_amd.polish.perform_stitch import perform_stitch  # noqa: E402


def device_fill_legs(pred, tmp, draft_fa, regions):
    """stitch_directory with fill against the host's file, then finish + take beside finish + fill + take on one handle."""
    import statistics

    from pepper_amd import h5
    from pepper_amd.polish.DeviceStitch import DeviceStitcher, _Held, _read_region, stitch_directory
    from pepper_amd.polish.perform_stitch import get_file_paths_from_directory
    runs = []
    host = open(os.path.join(tmp, "outf1") + "_pepper_polished.fa", "rb").read()
    for threads in (1, 8):
        for repeat in range(2):
            stats = {}
            t0 = time.perf_counter()
            out = stitch_directory(pred, os.path.join(tmp, "devf%d%d" % (threads, repeat)), threads, stats=stats, fill=draft_fa)
            dt = time.perf_counter() - t0
            runs.append({"merge": "device", "fill": True, "threads": threads, "repeat": repeat, "seconds": round(dt, 2),
                         "chunks_per_s": round(2 * regions / dt), "bases": os.path.getsize(out),
                         "equals_host": open(out, "rb").read() == host, "stats": stats})
    draft = open(draft_fa, "rb").read().split(b"\n")[1]
    with DeviceStitcher(0) as st:
        keys, held = [], _Held(st, "ctg0")
        for prediction_file in get_file_paths_from_directory(pred):
            with h5.File(prediction_file, 'r') as f:
                for name, start, end in f.list_polish_regions("ctg0"):
                    key, at = (prediction_file, name, start, end), 0
                    keys.append(key)
                    for block in _read_region(f, 'predictions/ctg0/ctg0-%d-%d' % (start, end)):
                        held.take(key, at, *block)
                        at += len(block[0])
        held.flush()
        legs = {}
        for leg, kw in (("finish_take", {}), ("finish_fill_take", {"fill": draft})):
            seconds = []
            for repeat in range(4):                          # (the first call grows the handle's tables)
                before = st.fill_totals["seconds"]
                t0 = time.perf_counter()
                sequence = st.finish("ctg0", 1, keys, **kw)
                seconds.append((time.perf_counter() - t0, st.fill_totals["seconds"] - before))
            legs[leg] = {"seconds": [round(s[0], 4) for s in seconds[1:]], "median": round(statistics.median(s[0] for s in seconds[1:]), 4),
                         "fill_call_seconds": [round(s[1], 4) for s in seconds[1:]], "letters": len(sequence), "stats": st.stats()}
        legs["ratio"] = round(legs["finish_fill_take"]["median"] / legs["finish_take"]["median"], 3)
        legs["fill_counts"] = st.last_fill_counts
        runs.append({"merge": "device", "fill": "one handle", **legs})
    return runs


def device_gate_legs(pred, tmp, draft_fa, regions, q):
    """stitch_directory with the gate against the host's files, then finish + take beside finish + gate + take on one handle."""
    import statistics

    from pepper_amd import h5
    from pepper_amd.polish.DeviceStitch import DeviceStitcher, _Held, _read_region, stitch_directory
    from pepper_amd.polish.perform_stitch import get_file_paths_from_directory
    runs = []
    for threads in (1, 8):
        host = [open(os.path.join(tmp, "outg%d" % threads) + suffix, "rb").read() for suffix in ("_pepper_polished.fa", "_pepper_polished.withheld.tsv")]
        for repeat in range(2):
            stats = {}
            t0 = time.perf_counter()
            out = stitch_directory(pred, os.path.join(tmp, "devg%d%d" % (threads, repeat)), threads, stats=stats, min_quality=q, draft=draft_fa)
            dt = time.perf_counter() - t0
            runs.append({"merge": "device", "min_quality": q, "threads": threads, "repeat": repeat, "seconds": round(dt, 2),
                         "chunks_per_s": round(2 * regions / dt), "bases": os.path.getsize(out),
                         "equals_host": open(out, "rb").read() == host[0],
                         "withheld_tsv_equals_host": open(out[:-len(".fa")] + ".withheld.tsv", "rb").read() == host[1], "stats": stats})
    draft = open(draft_fa, "rb").read().split(b"\n")[1]
    with DeviceStitcher(0) as st:
        keys, held = [], _Held(st, "ctg0")
        for prediction_file in get_file_paths_from_directory(pred):
            with h5.File(prediction_file, 'r') as f:
                for name, start, end in f.list_polish_regions("ctg0"):
                    key, at = (prediction_file, name, start, end), 0
                    keys.append(key)
                    for block in _read_region(f, 'predictions/ctg0/ctg0-%d-%d' % (start, end), True):
                        held.take(key, at, *block)
                        at += len(block[0])
        held.flush()
        legs = {}
        for leg, kw in (("finish_take", {}), ("finish_gate_take", {"min_quality": q, "draft": draft}),
                        ("finish_gate_take_withheld", {"min_quality": q, "draft": draft})):
            seconds = []
            for repeat in range(4):                          # (the first call grows the handle's tables)
                before = st.gate_totals["seconds"]
                t0 = time.perf_counter()
                sequence = st.finish("ctg0", 8, keys, **kw)
                if leg.endswith("withheld"):
                    st.withheld()
                seconds.append((time.perf_counter() - t0, st.gate_totals["seconds"] - before))
            legs[leg] = {"seconds": [round(s[0], 4) for s in seconds[1:]], "median": round(statistics.median(s[0] for s in seconds[1:]), 4),
                         "gate_call_seconds": [round(s[1], 4) for s in seconds[1:]], "letters": len(sequence), "stats": st.stats()}
        legs["ratio"] = round(legs["finish_gate_take"]["median"] / legs["finish_take"]["median"], 3)
        legs["gate_counts"] = st.last_gate_counts
        runs.append({"merge": "device", "min_quality": "one handle", **legs})
    return runs


def device_vcf_legs(pred, draft_fa):
    """On one handle that holds the job's rows with their phred, after one filled finish: the edit comparison with its copy back,
    pa_stitcher_variants with its copy back (the edit records are there), and the numpy twin on the same records; one warm-up
    and three timed calls each.  The device's records are checked against the twin's bytes."""
    import statistics

    from pepper_amd import h5
    from pepper_amd.polish import Variants
    from pepper_amd.polish.DeviceStitch import DeviceStitcher, _Held, _read_region
    from pepper_amd.polish.perform_stitch import get_file_paths_from_directory
    draft = open(draft_fa, "rb").read().split(b"\n")[1]
    with DeviceStitcher(0) as st:
        keys, held = [], _Held(st, "ctg0")
        for prediction_file in get_file_paths_from_directory(pred):
            with h5.File(prediction_file, 'r') as f:
                for name, start, end in f.list_polish_regions("ctg0"):
                    key, at = (prediction_file, name, start, end), 0
                    keys.append(key)
                    for block in _read_region(f, 'predictions/ctg0/ctg0-%d-%d' % (start, end), True):
                        held.take(key, at, *block)
                        at += len(block[0])
        held.flush()
        sequence = st.finish("ctg0", 1, keys, fill=draft)
        legs, results = {}, {}
        for leg, call in (("edits_take", lambda: st.edits(draft)), ("variants_take", lambda: st.variants(draft)),
                          ("twin", lambda: Variants.records_numpy(results["edits_take"], draft, sequence, True))):
            seconds = []
            for repeat in range(4):                          # (the first call grows the handle's tables)
                t0 = time.perf_counter()
                results[leg] = call()
                seconds.append(time.perf_counter() - t0)
            legs[leg] = {"seconds": [round(s, 4) for s in seconds[1:]], "median": round(statistics.median(seconds[1:]), 4)}
        legs["edit_records"], legs["variant_counts"] = len(results["edits_take"]), st.last_variant_counts
        legs["equals_twin"] = results["variants_take"].tobytes() == results["twin"][0].tobytes() and \
            st.last_variant_counts == results["twin"][1]
        legs["letters"], legs["stats"] = len(sequence), st.stats()
    return [{"merge": "device", "vcf": "one handle", **legs}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=65536)
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--device", action="store_true", help="also run the set through the device stitch")
    ap.add_argument("--qualities", action="store_true", help="also run the set with qualities on (FASTQ beside the FASTA)")
    ap.add_argument("--edits", action="store_true", help="also run the set with the edits on (.edits.tsv beside the FASTA)")
    ap.add_argument("--fill", action="store_true", help="also run the set with fill on (the draft where no row covered it)")
    ap.add_argument("--min-quality", type=int, default=0, help="also run the set with the gate on (only the edits with phred >= Q)")
    ap.add_argument("--vcf", action="store_true", help="with --device: time the variant normalisation beside the edit comparison and the twin")
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(dir=args.dir)
    try:
        pred = os.path.join(tmp, "pred")
        os.makedirs(pred)
        rng = np.random.default_rng(3)
        rng_phred = np.random.default_rng(4)               # (a stream of its own: the labels are the ones of every earlier run)
        stores = [DataStore(os.path.join(pred, "pepper_prediction_%d.hdf" % k), "w") for k in range(args.files)]
        regions = args.chunks // 2
        block = 256                                        # regions per write call
        idx = np.zeros((2 * block, 1000), np.int64)
        for r0 in range(0, regions, block):
            m = min(block, regions - r0)
            start = (r0 + np.arange(m)) * 1000
            start2 = np.repeat(start, 2)
            chunk = np.tile(np.array([0, 1]), m)
            position = start2[:, None] + (chunk * 950)[:, None] + np.arange(1000)[None, :]
            position[position > (start2 + 1200)[:, None]] = -1
            bases = rng.integers(0, 5, (2 * m, 1000)).astype(np.uint8)
            contigs = np.array([b"ctg0"] * (2 * m), dtype="S256")
            stores[(r0 // block) % args.files].write_predictions_block(contigs, start2, start2 + 1200, chunk, position, idx[:2 * m],
                                                                        bases, rng_phred.integers(0, 101, (2 * m, 1000)).astype(np.uint8))
        for s in stores:
            s.close()
        runs = []
        for numpy_form in (False, True):
            for threads in (1, 8):
                os.environ["PEPPER_AMD_STITCH_NUMPY"] = "1" if numpy_form else "0"
                t0 = time.perf_counter()
                out = perform_stitch(pred, os.path.join(tmp, "out%d%d" % (numpy_form, threads)), threads)
                dt = time.perf_counter() - t0
                runs.append({"merge": "numpy" if numpy_form else "library", "threads": threads, "seconds": round(dt, 2),
                             "chunks_per_s": round(2 * regions / dt), "bases": os.path.getsize(out)})
        if args.qualities:
            os.environ["PEPPER_AMD_STITCH_NUMPY"] = "0"
            for threads in (1, 8):
                t0 = time.perf_counter()
                out = perform_stitch(pred, os.path.join(tmp, "outq%d" % threads), threads, qualities=True)
                dt = time.perf_counter() - t0
                runs.append({"merge": "numpy", "qualities": True, "threads": threads, "seconds": round(dt, 2),
                             "chunks_per_s": round(2 * regions / dt), "bases": os.path.getsize(out),
                             "equals_fasta": open(out, "rb").read() == open(os.path.join(tmp, "out0%d" % threads) + "_pepper_polished.fa", "rb").read()})
        if args.edits or args.fill or args.min_quality or args.vcf:
            os.environ["PEPPER_AMD_STITCH_NUMPY"] = "0"
            draft_fa = os.path.join(tmp, "draft.fa")
            with open(draft_fa, "w") as fh:                 # as long as the positions reach
                fh.write(">ctg0\n" + np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(5).integers(0, 4, regions * 1000 + 2400)]
                         .tobytes().decode() + "\n")
        if args.edits:
            for threads in (1, 8):
                t0 = time.perf_counter()
                out = perform_stitch(pred, os.path.join(tmp, "oute%d" % threads), threads, edits=draft_fa)
                dt = time.perf_counter() - t0
                runs.append({"merge": "numpy", "edits": True, "threads": threads, "seconds": round(dt, 2),
                             "chunks_per_s": round(2 * regions / dt), "bases": os.path.getsize(out),
                             "edits_tsv_bytes": os.path.getsize(out[:-len(".fa")] + ".edits.tsv"),
                             "equals_fasta": open(out, "rb").read() == open(os.path.join(tmp, "out0%d" % threads) + "_pepper_polished.fa", "rb").read()})
        if args.fill:
            for threads in (1, 8):
                t0 = time.perf_counter()
                out = perform_stitch(pred, os.path.join(tmp, "outf%d" % threads), threads, fill=draft_fa)
                dt = time.perf_counter() - t0
                runs.append({"merge": "numpy", "fill": True, "threads": threads, "seconds": round(dt, 2),
                             "chunks_per_s": round(2 * regions / dt), "bases": os.path.getsize(out)})
        if args.min_quality:
            for threads in (1, 8):
                t0 = time.perf_counter()
                out = perform_stitch(pred, os.path.join(tmp, "outg%d" % threads), threads, min_quality=args.min_quality, draft=draft_fa)
                dt = time.perf_counter() - t0
                runs.append({"merge": "numpy", "min_quality": args.min_quality, "threads": threads, "seconds": round(dt, 2),
                             "chunks_per_s": round(2 * regions / dt), "bases": os.path.getsize(out),
                             "withheld_tsv_bytes": os.path.getsize(out[:-len(".fa")] + ".withheld.tsv")})
        if args.device:
            from pepper_amd.polish.DeviceStitch import stitch_directory
            host = {threads: open(os.path.join(tmp, "out0%d" % threads) + "_pepper_polished.fa", "rb").read() for threads in (1, 8)}
            for threads in (1, 8):
                for repeat in range(2):                    # (the first run loads the library and grows the handle's tables)
                    stats = {}
                    t0 = time.perf_counter()
                    out = stitch_directory(pred, os.path.join(tmp, "dev%d%d" % (threads, repeat)), threads, stats=stats)
                    dt = time.perf_counter() - t0
                    runs.append({"merge": "device", "threads": threads, "repeat": repeat, "seconds": round(dt, 2),
                                 "chunks_per_s": round(2 * regions / dt), "bases": os.path.getsize(out),
                                 "equals_host": open(out, "rb").read() == host[threads], "stats": stats})
            for threads in (1, 8) if args.qualities else ():
                host_fastq = open(os.path.join(tmp, "outq%d" % threads) + "_pepper_polished.fastq", "rb").read()
                for repeat in range(2):
                    stats = {}
                    t0 = time.perf_counter()
                    out = stitch_directory(pred, os.path.join(tmp, "devq%d%d" % (threads, repeat)), threads, stats=stats, qualities=True)
                    dt = time.perf_counter() - t0
                    fastq = open(out[:-len(".fa")] + ".fastq", "rb").read()
                    runs.append({"merge": "device", "qualities": True, "threads": threads, "repeat": repeat, "seconds": round(dt, 2),
                                 "chunks_per_s": round(2 * regions / dt), "bases": os.path.getsize(out),
                                 "equals_host": open(out, "rb").read() == host[threads], "fastq_equals_host": fastq == host_fastq,
                                 "fastq_bytes": len(fastq), "stats": stats})
            for threads in (1, 8) if args.edits else ():
                host_tsv = open(os.path.join(tmp, "oute%d" % threads) + "_pepper_polished.edits.tsv", "rb").read()
                for repeat in range(2):
                    stats = {}
                    t0 = time.perf_counter()
                    out = stitch_directory(pred, os.path.join(tmp, "deve%d%d" % (threads, repeat)), threads, stats=stats, edits=draft_fa)
                    dt = time.perf_counter() - t0
                    tsv = open(out[:-len(".fa")] + ".edits.tsv", "rb").read()
                    runs.append({"merge": "device", "edits": True, "threads": threads, "repeat": repeat, "seconds": round(dt, 2),
                                 "chunks_per_s": round(2 * regions / dt), "bases": os.path.getsize(out),
                                 "equals_host": open(out, "rb").read() == host[threads], "edits_tsv_equals_host": tsv == host_tsv,
                                 "edits_tsv_bytes": len(tsv), "stats": stats})
            if args.fill:
                runs.extend(device_fill_legs(pred, tmp, draft_fa, regions))
            if args.min_quality:
                runs.extend(device_gate_legs(pred, tmp, draft_fa, regions, args.min_quality))
            if args.vcf:
                runs.extend(device_vcf_legs(pred, draft_fa))
        from pepper_amd.hostinfo import usable_cpus
        print(json.dumps({"metric": "perform_stitch: prediction HDF5 -> FASTA (host" + (" and device" if args.device else "") + ")", "chunks": 2 * regions, "files": args.files,
                          "usable_cpus": usable_cpus(), "runs": runs}))
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
