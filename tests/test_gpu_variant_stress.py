"""The variant model where trained checkpoints live: confident heads and the stress families of weights in EVERY kernel
form variant_forward_chunk (api.hip) can pick, at call sizes that straddle every row tile, against the float64 restatement
(oracle/models_np.py variant_forward_f64) -- and the kernel labels each call really ran, asserted exactly.

Forms (environment read at model creation, restored right after):
  default          n <= 1024 the unit-split loops, n <= 3072 the small-call schedule, above it the big-call one
  small-call       PA_UNIT_SPLIT=0
  big-call         PA_SMALL_BATCH=0 PA_SMALL_ROWS=0 PA_UNIT_SPLIT=0 (what the benchmark and every production pass run)
  f32-loops        PA_SPLIT_REC=0
  f32              PA_SPLIT_GEMM=0 (the chain a checkpoint with a weight >= 64 takes)
  batch-invariant  pa_variant_set_batch_invariant(h, 1): the big-call kernels, in 32-row workgroups
Label sets: expected_labels() below, derived from form_of and the launch section of variant_forward_chunk.

A call of n windows is V-syn with min(n, 64) probes of weight_families.variant_case written over chosen rows -- row 0, row
n - 1, both sides of the last multiple of 32 / 64 / 128 / 256 below n and of 32 ... 1024, random rows for the rest -- and
only the probe rows are compared, so the oracle is evaluated once per (family, shape).

MEASURED (MI355X) max |p - p64| on the probe rows over all call sizes of a form (18; `default` 22), beside the float32
numpy restatement's own distance from float64 on the same probes (`own`: the larger of its probability and relative logit
distance).  The bar is 1e-4:

    family, shape              default    small-call big-call   f32-loops  f32        batch-inv. f32 numpy
    default_gain2, released    1.14e-06   1.05e-06   1.14e-06   1.01e-06   2.16e-06   1.45e-06   1.41e-06
    mixed_row_scales, released 4.42e-08   4.42e-08   4.42e-08   3.72e-08   3.72e-08   4.42e-08   4.14e-08
    heavy_tailed, released     2.61e-06   2.10e-06   2.55e-06   1.98e-06   3.96e-06   2.49e-06   1.61e-06
    large_bias, released       1.82e-07   1.80e-07   1.82e-07   1.68e-07   1.31e-07   2.00e-07   2.34e-07
    large_entries, released    1.78e-07   1.70e-07   1.78e-07   1.95e-07   8.50e-08   2.08e-07   1.54e-07
    near_tie_head, released    3.70e-08   3.70e-08   3.70e-08   3.70e-08   3.70e-08   3.70e-08   4.51e-08
    graded_head, released      4.94e-06   4.28e-06   4.94e-06   4.26e-06   9.53e-06   4.46e-06   2.28e-06
    confident_head, released   9.26e-06   7.65e-06   8.58e-06   1.25e-05   2.14e-05   1.20e-05   6.56e-06
    default, l2                6.05e-08   4.25e-08   4.44e-08   5.23e-08   4.25e-08   4.59e-08   4.84e-08
    confident_head, l2         1.13e-05   7.47e-06   9.71e-06   9.18e-06   1.46e-05   1.52e-05   8.97e-06
    default, f48w21            9.55e-08   9.55e-08   9.55e-08   9.55e-08   5.96e-08   8.15e-08   8.96e-08
    confident_head, f48w21     7.20e-06   7.20e-06   7.29e-06   3.71e-06   5.74e-06   2.64e-06   3.71e-06
The largest relative logit distance anywhere is 6.6e-6 (heavy_tailed, batch-invariant).  No form stands out: the big-call
loops are as close as the small-call ones, and the form furthest from float64 on the confident head is the exact-f32
chain (2.1e-5), whose linear_1 sums K = 16 896 in float32.  Float entry point: at most 1.8e-5 (confident_head, f32 chain);
golden of the reference's model class (variant_confident.npz): 1.2e-5 to 2.1e-5 in the six forms.

Each form was also broken on purpose once (every change in bounds; two builds, grouped so that no form's first failure
has two causes), and these tests run:
  * hi*lo term dropped in lstm_rec_h2_split_kernel / in lstm_dec_h2_kernel / in lstm_seed_h2_kernel: `default` / `big-call`
    and `batch-invariant` / `small-call` failed on default_gain2, heavy_tailed, large_entries, graded_head and
    confident_head (errors of 1.1e-4 to 8.4e-4 from that one term of one loop), and passed on mixed_row_scales,
    large_bias, near_tie_head and the gain-1 default -- the families every variant test was limited to before;
  * lo half zeroed in f32_to_h2_kernel (cvt_h2): `f32-loops` failed on the same five families, 1.4e-4 to 4.2e-4;
  * row n - 1 stored to row n - 2 in dense_small_kernel (head_softmax): `f32` failed in every family and shape at n = 2;
  * pad batches AND the last batch clamped to batch n - 2 in gemm_nt's fragment path: `default` and `f32` failed in every
    family at n = 2, every form of f48w21 and the float entry point as well.  (Clamping pad batches to batch 0 instead of
    n - 1 changes no stored value -- pad rows of Xp feed pad rows of the step loop only -- so no test can see it.)
The golden and the float entry point tests failed in both builds; forms that do not run a broken kernel stayed green.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import weight_families as wf
from oracle import models_np
from pepper_amd import _lib, synthetic

pytestmark = pytest.mark.gpu
TOL = 1e-4
ENV_KEYS = ("PA_SPLIT_REC", "PA_SPLIT_GEMM", "PA_SMALL_BATCH", "PA_SMALL_ROWS", "PA_UNIT_SPLIT", "PA_UNIT_SPLIT_SABOTAGE")
FORMS = {"default": {}, "small-call": {"PA_UNIT_SPLIT": "0"},
         "big-call": {"PA_SMALL_BATCH": "0", "PA_SMALL_ROWS": "0", "PA_UNIT_SPLIT": "0"},
         "f32-loops": {"PA_SPLIT_REC": "0"}, "f32": {"PA_SPLIT_GEMM": "0"}, "batch-invariant": {}}
SHAPES = {"released": {}, "l2": {"gru_layers": 2}, "f48w21": {"image_features": 48, "window": 21}}
SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 129, 255, 257, 511, 512, 513, 1023, 1024, 1025]
DEFAULT_SIZES = SIZES + [2048, 2049, 3072, 3073]
FLOAT_SIZES = [1, 65, 129]

CASES = [(family, "released", form) for family in ["default_gain2"] + wf.FAMILIES + wf.HEAD_FAMILIES for form in FORMS]
CASES += [(family, shape, form) for shape in ("l2", "f48w21") for family in ("default", "confident_head") for form in FORMS]
IDS = ["-".join(c) for c in CASES]


def expected_labels(form, n, features=26, float_input=False):
    """The kernel labels one call of n windows records (api.hip variant_forward_chunk).  The first layer contracts its
    input inside the step loop only for int8 summaries of at most 32 features; the unit split never does."""
    fused_in = features <= 32 and not float_input
    if form == "f32":
        first = {"lstm_rec_fused_in"} if fused_in else {"gemm_inproj_in"}
        return first | {"gemm_inproj", "lstm_rec", "gemm_linear_1", "gemm_linear_2to5", "head_softmax"}
    tail = {"gemm_h2_linear_1", "mlp_tail_h2"}
    if form == "f32-loops":
        first = {"lstm_rec_fused_in"} if fused_in else {"gemm_inproj_in"}
        return first | {"cvt_h2", "gemm_h2_inproj", "lstm_rec"} | tail
    if form == "default" and n <= 1024:
        return {"gemm_inproj_in", "lstm_rec_h2_split", "gemm_h2_inproj"} | tail
    first = {"lstm_rec_h2_fused_in"} if fused_in else {"gemm_inproj_in", "lstm_rec_h2"}
    if form in ("default", "small-call") and n <= 3072:
        return first | {"gemm_h2_inproj", "lstm_rec_h2"} | tail
    return first | {"lstm_dec_h2_fused"} | tail


class Model:
    """Raw C-ABI handle created under one form, profiling on."""

    def __init__(self, sd, form, gru_layers=1, window=33, image_features=26):
        self.lib = _lib.load()
        self.form, self.features = form, image_features
        cfg = _lib.VariantConfig(image_features, window, gru_layers, 3, 0, 0)
        names, data, numel, n, keep = _lib.marshal_state_dict(sd)
        self.h = ctypes.c_void_p()
        saved = {k: os.environ.get(k) for k in ENV_KEYS}
        try:
            for k in ENV_KEYS:
                os.environ.pop(k, None)
            os.environ.update(FORMS[form])
            _lib.check(self.lib.pa_variant_create(ctypes.byref(cfg), names, data, numel, n, None, ctypes.byref(self.h)))
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        if form == "batch-invariant":
            _lib.check(self.lib.pa_variant_set_batch_invariant(self.h, 1))

    def _fallbacks(self):
        v = ctypes.c_int64()
        _lib.check(self.lib.pa_variant_split_fallbacks(self.h, ctypes.byref(v)))
        return v.value

    def forward(self, x):
        """int8 windows through the host entry point, float windows through pa_variant_forward_device_f32 ->
        (probs, logits, labels of this call alone, the label set the call should have recorded)."""
        n = x.shape[0]
        before = self._fallbacks()
        _lib.check(self.lib.pa_profile_enable(self.h, 1))        # (also clears the labels of the call before)
        if x.dtype == np.int8:
            x = np.ascontiguousarray(x)
            probs, logits = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
            _lib.check(self.lib.pa_variant_forward_host(self.h, x.ctypes.data, n, probs.ctypes.data, logits.ctypes.data))
        else:
            assert x.dtype == np.float32
            xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
            pd = torch.empty((n, 3), dtype=torch.float32, device="cuda")
            ld = torch.empty_like(pd)
            torch.cuda.synchronize()
            _lib.check(self.lib.pa_variant_forward_device_f32(self.h, xd.data_ptr(), n, pd.data_ptr(), ld.data_ptr()))
            _lib.check(self.lib.pa_synchronize(self.h))
            probs, logits = pd.cpu().numpy(), ld.cpu().numpy()
        ran = set(_lib.profile_dict(self.h))
        float_input = x.dtype != np.int8
        want = expected_labels(self.form, n, self.features, float_input)
        if self._fallbacks() != before:
            # a split group did not meet (other work held the CUs): the call ran again on the small-call schedule
            want = want | expected_labels("small-call", n, self.features, float_input)
        return probs, logits, ran, want

    def close(self):
        if self.h:
            self.lib.pa_variant_destroy(self.h)
            self.h = None


def probe_rows(n, k, rng):
    """k distinct rows of a call of n windows: its ends, both sides of every row-tile boundary the kernels have, random rest."""
    must = [0, n - 1]
    for tile in (32, 64, 128, 256):
        m = (n - 1) // tile * tile             # the last multiple below n
        if m > 0:
            must += [m - 1, m]
    for b in (32, 64, 128, 256, 512, 1024):
        if b < n:
            must += [b - 1, b]
    must = list(dict.fromkeys(r for r in must if 0 <= r < n))[:k]
    rest = np.setdiff1d(np.arange(n), must)
    return np.array(must + list(rng.choice(rest, size=k - len(must), replace=False)), dtype=np.int64)


_CALLS = {}


def _call(case, n):
    """(x int8 [n, T, F], rows, k): V-syn neighbours with the first k probes of the case at the chosen rows; the neighbours
    and the rows depend on n and the shape alone, so they are drawn once."""
    sh = case["shape"]
    key = (n, sh["window"], sh["image_features"])
    if key not in _CALLS:
        k = min(n, len(case["x"]))
        _CALLS[key] = (wf.variant_windows(n, 1000 + n, sh["window"], sh["image_features"]), probe_rows(n, k, np.random.default_rng(n)), k)
    x, rows, k = _CALLS[key]
    x = x.copy()
    x[rows] = case["x"][:k]
    return x, rows, k


def _check_rows(p, l, p64, l64, what):
    """The assertions of one call on its probe rows -> (max |p - p64|, max |logit - l64| / max(1, max |l64|))."""
    assert np.isfinite(p).all() and np.isfinite(l).all(), what
    perr = float(np.abs(p - p64).max())
    lerr = float(np.abs(l - l64).max() / max(1.0, np.abs(l64).max()))
    assert perr <= TOL, (what, perr)
    assert lerr <= TOL, (what, lerr)
    assert np.abs(p.astype(np.float64).sum(1) - 1).max() < 1e-5, what
    top = np.sort(p64, axis=1)
    clear = (top[:, -1] - top[:, -2]) > 2 * TOL
    assert (p.argmax(1)[clear] == p64.argmax(1)[clear]).all(), what
    return perr, lerr


@pytest.mark.parametrize("family,shape,form", CASES, ids=IDS)
def test_every_form_at_every_row_tile(family, shape, form):
    """One (family, shape, form): a model, then every call size; per call the exact label set and, on the probe rows, the
    1e-4 bar on probabilities and (relative) logits against float64, rows summing to 1, the argmax wherever float64
    separates the two best classes by more than 2e-4."""
    case = wf.variant_case(family, **SHAPES[shape])
    assert case["own"] <= 1e-5, case["own"]            # a parity case (checked on the CPU too)
    m = Model(case["sd"], form, **case["shape"])
    worst = (0.0, 0.0)
    try:
        for n in (DEFAULT_SIZES if form == "default" else SIZES):
            x, rows, k = _call(case, n)
            p, l, ran, want = m.forward(x)
            assert ran == want, (family, shape, form, n, sorted(ran), sorted(want))
            assert np.isfinite(p).all() and np.isfinite(l).all(), (family, shape, form, n)       # every row, not the probes alone
            assert np.abs(p.astype(np.float64).sum(1) - 1).max() < 1e-5, (family, shape, form, n)
            errs = _check_rows(p[rows], l[rows], case["p64"][:k], case["l64"][:k], (family, shape, form, n))
            worst = (max(worst[0], errs[0]), max(worst[1], errs[1]))
    finally:
        m.close()
    print(f"MEASURED {family}-{shape}-{form}: p {worst[0]:.2e} logit {worst[1]:.2e}  f32 restatement {case['own']:.2e}")


def test_label_sets_show_the_switch_points():
    """The table expected_labels() encodes, spelled out where the schedules change hands (released shape, int8 calls)."""
    assert "lstm_rec_h2_split" in expected_labels("default", 1024)
    assert "lstm_rec_h2" in expected_labels("default", 1025) and "lstm_rec_h2_split" not in expected_labels("default", 1025)
    assert "lstm_rec_h2" in expected_labels("default", 3072) and "lstm_dec_h2_fused" not in expected_labels("default", 3072)
    assert "lstm_dec_h2_fused" in expected_labels("default", 3073) and "lstm_rec_h2" not in expected_labels("default", 3073)
    assert expected_labels("default", 512) == {"gemm_inproj_in", "lstm_rec_h2_split", "gemm_h2_inproj", "gemm_h2_linear_1", "mlp_tail_h2"}
    assert expected_labels("small-call", 512) == {"lstm_rec_h2_fused_in", "gemm_h2_inproj", "lstm_rec_h2", "gemm_h2_linear_1", "mlp_tail_h2"}
    assert expected_labels("big-call", 512) == {"lstm_rec_h2_fused_in", "lstm_dec_h2_fused", "gemm_h2_linear_1", "mlp_tail_h2"}
    assert expected_labels("batch-invariant", 1) == expected_labels("big-call", 1)
    assert expected_labels("f32-loops", 512) == {"lstm_rec_fused_in", "lstm_rec", "cvt_h2", "gemm_h2_inproj", "gemm_h2_linear_1", "mlp_tail_h2"}
    assert expected_labels("f32", 512) == {"lstm_rec_fused_in", "gemm_inproj", "lstm_rec", "gemm_linear_1", "gemm_linear_2to5", "head_softmax"}
    assert not any("_h2" in k for k in expected_labels("f32", 512) | expected_labels("f32", 512, 48) | expected_labels("f32", 5, 26, True))
    # more than 32 features, or float windows: no fused-in form exists
    for form in FORMS:
        for kw in (dict(features=48), dict(float_input=True)):
            want = expected_labels(form, 2000, **kw)
            assert "gemm_inproj_in" in want and not any(k.endswith("_fused_in") for k in want), (form, kw)


@pytest.mark.parametrize("form", ["default", "f32"])
@pytest.mark.parametrize("family", ["default_gain2", "confident_head"])
def test_float_entry_point(family, form):
    """pa_variant_forward_device_f32 on the int8 values as floats and on 0.37 times them (no longer integers): the
    projection GEMM reads the floats, no fused-in loop runs, the same bar against float64 of the same floats."""
    case = wf.variant_case(family)
    scaled = (case["x"].astype(np.float32) * np.float32(0.37)).astype(np.float32)
    p37, l37 = models_np.variant_forward_f64(case["sd"], scaled)
    m = Model(case["sd"], form)
    try:
        for n in FLOAT_SIZES:
            x, rows, k = _call(case, n)
            for tag, xf, p64, l64 in (("x1", x.astype(np.float32), case["p64"], case["l64"]),
                                      ("x0.37", (x.astype(np.float32) * np.float32(0.37)).astype(np.float32), p37, l37)):
                p, l, ran, want = m.forward(xf)
                assert ran == want, (family, form, n, tag, sorted(ran), sorted(want))
                assert "gemm_inproj_in" in ran and not any(k_.endswith("_fused_in") for k_ in ran), ran
                errs = _check_rows(p[rows], l[rows], p64[:k], l64[:k], (family, form, n, tag))
                print(f"MEASURED float {family}-{form}-{n}-{tag}: p {errs[0]:.2e} logit {errs[1]:.2e}")
    finally:
        m.close()


def test_confident_head_matches_the_reference_golden(golden_dir):
    """tests/golden/variant_confident.npz: the reference's own model class on the confident head (make_golden.py
    make_variant(head_scale=12)), every form within 1e-4 of it and the same call wherever its two best probabilities differ
    by more than 2e-4."""
    g = np.load(os.path.join(golden_dir, "variant_confident.npz"))
    sd = synthetic.variant_state_dict(seed=int(g["seed"]), gain=float(g["gain"]))
    sd["output_layer_type.weight"] *= np.float32(g["head_scale"])
    sd["output_layer_type.bias"] *= np.float32(g["head_scale"])
    top = np.sort(g["probs"], axis=1)
    clear = (top[:, -1] - top[:, -2]) > 2 * TOL
    assert clear.sum() > 50 and np.abs(g["logits"]).max() > 10
    for form in FORMS:
        m = Model(sd, form)
        try:
            p, l, ran, want = m.forward(g["images"])
        finally:
            m.close()
        assert ran == want, (form, sorted(ran), sorted(want))
        perr, lerr = wf.errors(p, l, g["probs"], g["logits"])
        print(f"GOLDEN {form}: p {perr:.2e} logit {lerr:.2e}")
        assert perr <= TOL and lerr <= TOL, (form, perr, lerr)
        assert (p.argmax(1)[clear] == g["probs"].argmax(1)[clear]).all(), form
