"""Stress families of variant-model weights for the split-f16 arithmetic: the seeded-uniform
recipe of pepper_amd.synthetic only scales ONE distribution; a trained checkpoint has rows of very different
magnitude side by side, heavy tails and the odd large bias.  Each family starts from the PyTorch-default init and
reshapes it; `near_tie_head` makes the three class scores almost equal so that tiny logit errors would flip calls.
Also a numpy emulation of the product's arithmetic (every contraction as hi*hi + hi*lo + lo*hi on f16 halves) so the
families can be judged on the CPU before a GPU sees them.

Variant head families (HEAD_FAMILIES, on the gain-2 recipe): at gain 1 the three logits hardly move with the input (max
|logit| 0.09, every probability about 1/3, one class called on 63 of 64 probes), so a wrong LSTM is invisible in the
probabilities.  `graded_head` (output_layer_type x 4) reaches |logit| 7.2 and best probabilities 0.41 .. 0.973,
`confident_head` (x 12) |logit| 21.7, calls split 3 / 17 / 44 and best probabilities 0.57 .. 0.99999 on the 64 probes of
variant_case (0.40 .. 0.99999 on 96).  What each head can catch -- variant_forward_emulated against float64 on the first
12 probes (seed 70, probes seed 7), as max |dp| / max relative |dlogit|, with the product's three terms and with the lo
halves of every product dropped (terms=1):
    family              hi*hi + hi*lo + lo*hi    hi*hi only
    default, gain 1     8.2e-8 / 3.9e-7          5.8e-5 / 3.3e-4
    mixed_row_scales    4.0e-8 / 1.3e-7          2.9e-6 / 1.3e-5     (passes the 1e-4 bar with the lo halves gone)
    near_tie_head       3.7e-8 / 1.2e-7          3.7e-8 / 7.2e-5     (so does this)
    graded_head         1.6e-6 / 7.3e-6          2.4e-3 / 4.1e-3
    confident_head      1.5e-6 / 7.3e-6          2.3e-3 / 4.1e-3
A variant family or shape is a parity case only while the float32 restatement stays within 1e-5 of float64 on the 64
probes (variant_case `own`, the larger of max |dp| and max relative |dlogit|).  Measured:
    default 6.3e-8   default_gain2 1.4e-6   mixed_row_scales 4.1e-8   heavy_tailed 1.6e-6   large_bias 2.3e-7
    large_entries 1.5e-7   near_tie_head 4.5e-8   graded_head 2.3e-6   confident_head 6.6e-6
    two layers: default 4.8e-8, confident_head 9.0e-6     48 features x 21 rows: default 9.0e-8, confident_head 3.7e-6
so confident_head keeps head x 12 at every shape (no shape needed a smaller scale).

Polish families (make_polish, POLISH_FAMILIES): the same idea for the bi-GRU polish model, plus the head of a trained
checkpoint -- `confident_head` (dense1 x 40) puts phred between 1 and 100 with the accumulator at exactly 1.0 / 2.0 on
about a tenth of the positions, `graded_head` (dense1.weight x 12) spreads phred over 1 .. 48.  The 1900-step recurrence
with its hidden carry turns chaotic when the GRU matrices grow, so a family is a parity case only while the float32
restatement itself stays within 1e-5 of the float64 one on the test's own chunks (polish_case: seed 70, 20 chunks of
P-syn seed 2024).  Measured max |acc_f32 - acc_f64|:
    default 1.5e-7   graded_head 1.2e-6   confident_head 4.1e-6   near_tie_head 7.9e-8   large_bias 2.1e-7
    mixed_row_scales  top 0: 8.2e-8   0.5: 8.7e-8   1.0: 1.3e-7   1.2: 1.5e-7 (kept)   1.5: 2.3e-1   2.0: 4.2e-1
    large_entries     rate 1e-4: 3.1e-7   2e-4: 3.2e-6   3e-4: 1.9e-6 (kept)   5e-4: 3.2e-5
    confident_head at 3 classes 4.4e-6, 7 classes 3.8e-6, two GRU layers 2.5e-6, hidden size 256 (6 chunks) 4.2e-6
so all six are parity cases (tests/test_weight_families_cpu.py holds each to 1e-5)."""
import numpy as np

from pepper_amd import synthetic

FAMILIES = ["mixed_row_scales", "heavy_tailed", "large_bias", "large_entries", "near_tie_head"]
# heads of a trained checkpoint, on the gain-2 recipe (kept out of FAMILIES: the parametrisations over that list, the
# 16 384-window batch-invariance test among them, must not grow)
HEAD_FAMILIES = ["graded_head", "confident_head"]
HEAD_SCALES = {"graded_head": 4.0, "confident_head": 12.0}


def make(name, seed, head_scale=None, **shape_kw):
    """Variant checkpoints; shape_kw: gru_layers, image_features, window.  `default` is the unchanged gain-1 recipe,
    `default_gain2` the gain-2 one, the HEAD_FAMILIES scale output_layer_type (weight and bias) of the gain-2 recipe by
    HEAD_SCALES (or by head_scale)."""
    if name == "default_gain2" or name in HEAD_SCALES:
        sd = synthetic.variant_state_dict(seed=seed, gain=2.0, **shape_kw)
        scale = np.float32(HEAD_SCALES.get(name, 1.0) if head_scale is None else head_scale)
        sd["output_layer_type.weight"] *= scale
        sd["output_layer_type.bias"] *= scale
        return sd
    sd = synthetic.variant_state_dict(seed=seed, gain=1.0, **shape_kw)
    rng = np.random.default_rng([seed, 99])
    shapes = {s[0]: s[2] for s in synthetic.variant_param_shapes(**shape_kw)}
    if name == "default":
        pass
    elif name == "mixed_row_scales":
        # per output row: 1e-3 .. 16 x the default bound for the LSTM matrices (|w| from ~6e-5 to ~1 side by side),
        # 1e-3 .. 3 x for the dense layers (their fan-in is up to 16896: larger rows only saturate everything)
        for k, v in sd.items():
            if v.ndim == 2:
                top = 1.2 if ("encoder" in k or "decoder" in k) else 0.5
                v *= (10.0 ** rng.uniform(-3.0, top, size=(v.shape[0], 1))).astype(np.float32)
    elif name == "heavy_tailed":
        for k, v in sd.items():
            if v.ndim == 2:
                t = rng.standard_t(2.0, size=v.shape) * 0.5
                sd[k] = (np.clip(t, -40.0, 40.0) * shapes[k]).astype(np.float32)
    elif name == "large_bias":
        for k, v in sd.items():
            if v.ndim == 1:
                v *= 50.0
    elif name in ("large_entries", "near_f16_limit"):
        # a sprinkle of large entries in the LSTM matrices (their inputs are bounded -- int8 summaries, h in (-1, 1) -- so
        # the f16 range constrains the weights alone).  large_entries: +-50, just under api.hip's kSplitMaxWeight, the
        # largest weights the split-f16 kernels are asked to carry.  near_f16_limit: +-2.0e4 (x 2.89 gate pre-scale =
        # 5.8e4 < 65504): such a checkpoint runs on the exact-f32 kernels, and with pre-activation terms of 1e4 .. 1e6
        # float32 arithmetic itself is only good to ~1e-3 on an unsaturated gate, whatever the summation order: the
        # family is a robustness probe (finite, saturating), not a parity case.
        mag = 50.0 if name == "large_entries" else 2.0e4
        for k, v in sd.items():
            if v.ndim == 2 and ("encoder" in k or "decoder" in k):
                hit = rng.random(v.shape) < 5e-4
                v[hit] = rng.choice([-mag, mag], size=int(hit.sum())).astype(np.float32)
    elif name == "near_tie_head":
        w, b = sd["output_layer_type.weight"], sd["output_layer_type.bias"]
        w[1] = w[0] * (1.0 + 1e-4)
        w[2] = w[0] * (1.0 - 2e-4)
        b[1] = b[0] + 1e-5
        b[2] = b[0] - 1e-5
    else:
        raise KeyError(name)
    return sd


POLISH_FAMILIES = ["graded_head", "confident_head", "near_tie_head", "mixed_row_scales", "large_bias", "large_entries"]
POLISH_MIXED_TOP = 1.2        # mixed_row_scales: per-row factors 10 ** U(-3, top) on the GRU matrices
POLISH_SPRINKLE_RATE = 3e-4   # large_entries: share of GRU matrix entries set to +-50


def make_polish(name, seed, top=None, rate=None, **shape_kw):
    """Polish checkpoints (pepper_amd.synthetic.polish_state_dict(gain=1) reshaped); shape_kw: hidden, num_classes,
    gru_layers.  `default` is the unchanged recipe."""
    sd = synthetic.polish_state_dict(seed=seed, gain=1.0, **shape_kw)
    rng = np.random.default_rng([seed, 98])
    gru = [k for k, v in sd.items() if v.ndim == 2 and k.startswith("gru_")]
    if name == "default":
        pass
    elif name == "graded_head":
        sd["dense1.weight"] *= 12.0
    elif name == "confident_head":
        sd["dense1.weight"] *= 40.0
        sd["dense1.bias"] *= 40.0
    elif name == "near_tie_head":
        w, b = sd["dense1.weight"], sd["dense1.bias"]
        for c in range(1, w.shape[0]):
            sign = 1.0 if c % 2 else -1.0
            w[c] = w[0] * np.float32(1.0 + sign * c * 1e-4)
            b[c] = b[0] + np.float32(sign * 1e-5)
    elif name == "mixed_row_scales":
        top = POLISH_MIXED_TOP if top is None else top
        for k in gru:
            sd[k] *= (10.0 ** rng.uniform(-3.0, top, size=(sd[k].shape[0], 1))).astype(np.float32)
    elif name == "large_bias":
        for k, v in sd.items():
            if v.ndim == 1:
                v *= 20.0
    elif name == "large_entries":
        rate = POLISH_SPRINKLE_RATE if rate is None else rate
        for k in gru:
            hit = rng.random(sd[k].shape) < rate
            sd[k][hit] = rng.choice([-50.0, 50.0], size=int(hit.sum())).astype(np.float32)
    else:
        raise KeyError(name)
    return sd


def polish_stress_chunks(n, seed):
    """n chunks of P-syn, one of them zero from position 300 on (the padded tail chunk_images produces)."""
    x = synthetic.polish_chunks(n, seed=seed)
    x[min(1, n - 1), 300:] = 0
    return x


POLISH_SEED, POLISH_CHUNK_SEED, POLISH_CHUNKS = 70, 2024, 20
_POLISH_CASES = {}


def polish_case(name, n=POLISH_CHUNKS, **shape_kw):
    """One family (or `default`) at one model shape on the stress chunks, restated once per process in float64 and in
    float32: dict(sd, x, acc64, counts, acc32, own) with own = max |acc32 - acc64|, the float32 restatement's own distance
    from exact arithmetic.  Shared by the CPU checks and the GPU tests; callers leave the arrays unchanged."""
    import warnings
    from oracle import models_np
    key = (name, n, tuple(sorted(shape_kw.items())))
    if key not in _POLISH_CASES:
        sd = make_polish(name, POLISH_SEED, **shape_kw)
        x = polish_stress_chunks(n, POLISH_CHUNK_SEED)
        H, L = shape_kw.get("hidden", synthetic.POLISH_HIDDEN), shape_kw.get("gru_layers", 1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # exp overflow inside the float32 sigmoid of saturated gates
            acc64, counts = models_np.polish_predict_chunks_f64(sd, x, H, gru_layers=L)
            _, _, inter = models_np.polish_predict_chunks(sd, x, H, gru_layers=L, return_intermediates=True)
        _POLISH_CASES[key] = dict(sd=sd, x=x, acc64=acc64, counts=counts, acc32=inter["acc"],
                                  own=float(np.abs(inter["acc"] - acc64).max()))
    return _POLISH_CASES[key]


def polish_phred_from_acc(acc, counts):
    """Labels, phred and t = f32(1 - f32(best / counts)) from a float32 accumulator, the finalize step restated in float64:
    ph = -10 log10(t), 100 where t == 0, truncated to uint8.  -> (labels uint8, phred uint8, ph float64, t float32)."""
    acc = np.asarray(acc, np.float32)
    labels = acc.argmax(axis=2).astype(np.uint8)        # first maximum wins
    best = acc.max(axis=2)
    q = (best / np.asarray(counts, np.float32)).astype(np.float32)
    t = (np.float32(1.0) - q).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        ph = -10.0 * np.log10(t.astype(np.float64))      # (NaN where t < 0: best > counts, which no softmax sum gives)
    ph[t == 0] = 100.0
    return labels, np.floor(np.where(t < 0, 0.0, ph)).astype(np.uint8), ph, t


def stress_windows(n, seed, window=synthetic.VARIANT_WINDOW, features=synthetic.VARIANT_FEATURES):
    """V-syn windows whose rows 0 to 2 are the int8 extremes 127 / -128 / 0.  V-syn fills 26 feature columns: a wider
    summary repeats the columns of a second draw in the rest, so that no input weight is multiplied by zeros only."""
    x = variant_windows(n, seed, window, features)
    x[0] = 127
    x[1] = -128
    x[2] = 0
    return x


def variant_windows(n, seed, window=synthetic.VARIANT_WINDOW, features=synthetic.VARIANT_FEATURES):
    x = synthetic.variant_windows(n, seed=seed, window=window, features=max(features, synthetic.VARIANT_FEATURES))
    if features > synthetic.VARIANT_FEATURES:
        more = synthetic.variant_windows(n, seed=seed + 1, window=window)
        for c in range(synthetic.VARIANT_FEATURES, features):
            x[:, :, c] = more[:, :, c % synthetic.VARIANT_FEATURES]
    return x[:, :, :features]


VARIANT_SEED, VARIANT_PROBE_SEED, VARIANT_PROBES = 70, 7, 64
_VARIANT_CASES = {}


def variant_case(name, n_probes=VARIANT_PROBES, **shape_kw):
    """One variant family (or `default` / `default_gain2`) at one model shape (gru_layers, image_features, window) on the
    probe windows, restated once per process in float64 and in float32: dict(sd, x, p64, l64, p32, l32, own, shape) with
    own = errors(p32, l32, p64, l64), the float32 restatement's own distance from exact arithmetic.  Shared by the CPU
    checks and the GPU tests; callers leave the arrays unchanged."""
    import warnings
    from oracle import models_np
    key = (name, n_probes, tuple(sorted(shape_kw.items())))
    if key not in _VARIANT_CASES:
        L = shape_kw.get("gru_layers", 1)
        T = shape_kw.get("window", synthetic.VARIANT_WINDOW)
        F = shape_kw.get("image_features", synthetic.VARIANT_FEATURES)
        sd = make(name, VARIANT_SEED, **shape_kw)
        x = stress_windows(n_probes, VARIANT_PROBE_SEED, window=T, features=F)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # exp overflow inside the float32 sigmoid of saturated gates
            p64, l64 = models_np.variant_forward_f64(sd, x, gru_layers=L)
            p32, inter = models_np.variant_forward(sd, x, gru_layers=L, return_intermediates=True)
        _VARIANT_CASES[key] = dict(sd=sd, x=x, p64=p64, l64=l64, p32=p32, l32=inter["logits"],
                                   own=max(errors(p32, inter["logits"], p64, l64)), shape=dict(gru_layers=L, window=T, image_features=F))
    return _VARIANT_CASES[key]


# ---- numpy emulation of the split-f16 product ----------------------------------------------------------------------
def split(v):
    hi = v.astype(np.float16)
    lo = (v.astype(np.float32) - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def mm3(a, w, terms=3):
    """a [M,K] f32, w [N,K] f32 -> a w^T with hi*hi + hi*lo + lo*hi (products exact, accumulation not rounded); terms=1:
    hi*hi alone, a kernel that lost its lo halves."""
    ah, al = split(a)
    wh, wl = split(w)
    if terms == 1:
        return (ah @ wh.T).astype(np.float32)
    assert terms == 3
    return (ah @ wh.T + ah @ wl.T + al @ wh.T).astype(np.float32)


def variant_forward_emulated(sd, images, terms=3, gru_layers=1):
    """The product's arithmetic in numpy (terms=3); terms=1 drops the lo halves of every product -- the gross error the
    head families must make visible (module docstring)."""
    f4 = np.float32
    mm = lambda a, w: mm3(a, w, terms)   # noqa: E731
    sig = lambda v: (1.0 / (1.0 + np.exp(-np.clip(v.astype(np.float64), -700, 700)))).astype(f4)   # noqa: E731

    def direction(x, w_ih, w_hh, b_ih, b_hh, reverse):
        B, T, F = x.shape
        H = w_hh.shape[1]
        h, c = np.zeros((B, H), f4), np.zeros((B, H), f4)
        y = np.zeros((B, T, H), f4)
        xp = mm(x.reshape(B * T, F), w_ih).reshape(B, T, 4 * H) + (b_ih + b_hh)
        for t in (range(T - 1, -1, -1) if reverse else range(T)):
            g = xp[:, t] + mm(h, w_hh)
            c = sig(g[:, H:2 * H]) * c + sig(g[:, :H]) * np.tanh(g[:, 2 * H:3 * H])
            h = (sig(g[:, 3 * H:]) * np.tanh(c)).astype(f4)
            y[:, t] = h
        return y

    x = np.asarray(images).astype(f4)
    for prefix in ("encoder", "decoder"):
        for layer in range(gru_layers):
            x = np.concatenate([direction(x, sd[f"{prefix}.weight_ih_l{layer}{s}"], sd[f"{prefix}.weight_hh_l{layer}{s}"],
                                          sd[f"{prefix}.bias_ih_l{layer}{s}"], sd[f"{prefix}.bias_hh_l{layer}{s}"], rev)
                                for s, rev in (("", False), ("_reverse", True))], axis=2)
    a = x.reshape(x.shape[0], -1)
    from oracle.models_np import selu, softmax
    for name in ("linear_1", "linear_2", "linear_3", "linear_4", "linear_5"):
        a = selu(mm(a, sd[f"{name}.weight"]) + sd[f"{name}.bias"])
    logits = (a.astype(np.float64) @ sd["output_layer_type.weight"].astype(np.float64).T + sd["output_layer_type.bias"]).astype(f4)
    return softmax(logits, axis=1), logits


def errors(probs, logits, ref_probs, ref_logits):
    """(max |dp|, max |dlogit| / max(1, max |logit|))."""
    return (float(np.abs(probs - ref_probs).max()),
            float(np.abs(logits - ref_logits).max() / max(1.0, np.abs(ref_logits).max())))
