"""bench.py's plain run on the GPU: set-up, warm-up, the timed steps and the line, nothing else.  The CPU baselines, the
device-resident and default-batch legs, the secondary block and the other models' extra legs run only under --full, and only a
--full run writes the whole record.  Each run is a child process with a deadline."""
import importlib.util
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
HEADLINE = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype")


def _record_path():
    spec = importlib.util.spec_from_file_location("bench_module", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return os.path.join(REPO, mod.FULL_RECORD)


def _plain(args):
    record = _record_path()
    before = os.stat(record).st_mtime_ns if os.path.exists(record) else None
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    for key in HEADLINE:
        assert line.get(key) is not None, key
    assert line["steps"] == int(args[args.index("--steps") + 1]) and line["warmup"] == int(args[args.index("--warmup") + 1])
    assert "full_record" not in line
    assert (os.stat(record).st_mtime_ns if os.path.exists(record) else None) == before          # no record written
    return line, wall


def test_plain_variant_run_times_the_headline_only():
    line, wall = _plain(["--gpus", "1", "--steps", "2", "--warmup", "1"])
    assert line["unit"] == "windows/s" and line["value"] > 0 and line["roofline"]["kernel"]
    for key in ("cpu_baseline", "cpu_baseline_single_process", "speedup_vs_cpu_baseline", "device_resident", "batch512",
                "secondary_summary"):
        assert key not in line, key
    assert wall < 120, wall          # the extra legs took minutes; set-up and three steps take seconds


@pytest.mark.parametrize("model, extra_keys", [
    ("polish", ("cpu_baseline", "device_resident", "batch128")),
    ("realign", ("cpu_baseline", "reads_per_s_4_worker_threads", "reads_per_s_one_region_call", "ms_per_60_read_region")),
    ("encoder", ("cpu_baseline", "host_buffers_one_call", "packed_host_fed", "concurrent_handles")),
    ("polish-encoder", ("cpu_baseline", "host_buffers_one_call", "rows_region0")),
])
def test_plain_model_runs_leave_their_extra_legs_to_full(model, extra_keys):
    line, _ = _plain(["--model", model, "--steps", "2", "--warmup", "1"])
    assert line["value"] > 0
    for key in extra_keys:
        assert key not in line, key
