"""Cost of the batch-invariant mode: one JSON line per mode (off, on) with
  variant windows/s at 16 384-window passes through pa_variant_forward_host,
  ms per variant call at 512 and 1 024 windows (host entry point, median),
  polish chunks/s at 16 384 chunks and ms at 128 chunks (pa_polish_predict_host, median).

    python tools/bench_batch_invariant.py [--reps N]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from pepper_amd import _lib, synthetic  # noqa: E402


def _median_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def _pinned(a):
    """Page-locked copy of a host array (the host entry points overlap their copies only from such buffers)."""
    import torch
    t = torch.empty(a.shape, dtype={np.int8: torch.int8, np.uint8: torch.uint8, np.float32: torch.float32}[a.dtype.type],
                    pin_memory=True)
    t.numpy()[...] = a
    return t


def measure(mode, reps):
    import torch
    lib = _lib.load()
    torch.cuda.set_device(0)
    out = {"batch_invariant": bool(mode)}
    # ---- variant
    sd = synthetic.variant_state_dict(seed=3, gain=2.0)
    cfg = _lib.VariantConfig(26, 33, 1, 3, 0, 0)
    names, data, numel, n, keep = _lib.marshal_state_dict(sd)
    h = ctypes.c_void_p()
    _lib.check(lib.pa_variant_create(ctypes.byref(cfg), names, data, numel, n, None, ctypes.byref(h)))
    _lib.check(lib.pa_variant_set_batch_invariant(h, int(mode)))
    x = _pinned(synthetic.variant_windows(4 * 16384, seed=4))
    probs = _pinned(np.empty((4 * 16384, 3), np.float32))

    def run(k):
        return lambda: _lib.check(lib.pa_variant_forward_host(h, x.data_ptr(), k, probs.data_ptr(), None))
    ms = _median_ms(run(4 * 16384), reps)
    out["variant_windows_per_s_16384_passes"] = round(4 * 16384 / (ms / 1e3))
    out["variant_ms_512"] = round(_median_ms(run(512), 5 * reps), 4)
    out["variant_ms_1024"] = round(_median_ms(run(1024), 5 * reps), 4)
    # where a 512-window call's time goes (HIP events around each launch, one call)
    _lib.check(lib.pa_profile_enable(h, 1))
    run(512)()
    out["variant_512_kernel_ms"] = {k: round(v["ms"], 4) for k, v in _lib.profile_dict(h).items()}
    _lib.check(lib.pa_profile_enable(h, 0))
    lib.pa_variant_destroy(h)
    # ---- polish
    psd = synthetic.polish_state_dict(seed=5, gain=2.0)
    pcfg = _lib.PolishConfig(10, 128, 1, 5, 1000, 100, 50, 50, 0, 0)
    names, data, numel, n, keep = _lib.marshal_state_dict(psd)
    ph = ctypes.c_void_p()
    _lib.check(lib.pa_polish_create(ctypes.byref(pcfg), names, data, numel, n, None, ctypes.byref(ph)))
    _lib.check(lib.pa_polish_set_batch_invariant(ph, int(mode)))
    img = _pinned(synthetic.polish_chunks(16384, seed=6))
    lab = _pinned(np.empty((16384, 1000), np.uint8))
    phr = _pinned(np.empty((16384, 1000), np.uint8))

    def prun(k):
        return lambda: _lib.check(lib.pa_polish_predict_host(ph, img.data_ptr(), k, lab.data_ptr(), phr.data_ptr(), None))
    ms = _median_ms(prun(16384), max(3, reps // 2))
    out["polish_chunks_per_s_16384"] = round(16384 / (ms / 1e3))
    out["polish_ms_128"] = round(_median_ms(prun(128), reps), 3)
    lib.pa_polish_destroy(ph)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    for mode in (0, 1):
        print(json.dumps(measure(mode, args.reps)), flush=True)


if __name__ == "__main__":
    main()
