"""CPU leg of the weight-family stress test (tests/weight_families.py): the numpy emulation of the product's
arithmetic -- every contraction as hi*hi + hi*lo + lo*hi on f16 halves of f32 operands -- against the float64
restatement.  The GPU legs are tests/test_gpu_arith_modes.py::test_split_arithmetic_on_weight_families (the unit-split
form) and tests/test_gpu_variant_stress.py (every kernel form, with the head families)."""
import warnings

import numpy as np
import pytest

import weight_families as wf
from oracle import models_np


@pytest.mark.parametrize("family", ["mixed_row_scales", "heavy_tailed", "large_bias"])
def test_emulated_split_arithmetic_meets_the_bar(family):
    sd = wf.make(family, 70)
    x = wf.stress_windows(6, 7)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p64, l64 = models_np.variant_forward_f64(sd, x)
        p32, inter = models_np.variant_forward(sd, x, return_intermediates=True)
        pe, le = wf.variant_forward_emulated(sd, x)
    assert np.isfinite(pe).all()
    # the float32 restatement and the emulated split arithmetic are both far inside 1e-4 of exact arithmetic
    assert max(wf.errors(p32, inter["logits"], p64, l64)) < 2e-5
    assert max(wf.errors(pe, le, p64, l64)) < 2e-5


def test_why_large_weights_leave_the_split_path():
    """The absolute floor of the split format (2^-25 on an activation) times a weight in the thousands is visible: the
    emulated split arithmetic misses the bar at |w| = 2e4 while the float32 restatement does not -- which is why
    pa_*_create sends such checkpoints to the exact-f32 kernels (api.hip kSplitMaxWeight = 64)."""
    sd = wf.make("near_f16_limit", 70)
    x = wf.stress_windows(6, 7)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p64, l64 = models_np.variant_forward_f64(sd, x)
        p32, inter = models_np.variant_forward(sd, x, return_intermediates=True)
        pe, le = wf.variant_forward_emulated(sd, x)
    assert max(wf.errors(p32, inter["logits"], p64, l64)) < 2e-5
    assert max(wf.errors(pe, le, p64, l64)) > 1e-4


# ---- variant head families and shapes (GPU leg: tests/test_gpu_variant_stress.py) ------------------------------------
VARIANT_SHAPES = [{}, {"gru_layers": 2}, {"image_features": 48, "window": 21}]


@pytest.mark.parametrize("family", ["default", "default_gain2"] + wf.FAMILIES + wf.HEAD_FAMILIES)
def test_variant_family_stays_conditioned(family):
    """A family is a parity case only while the float32 restatement itself stays within 1e-5 of float64 on the probe
    windows (measured distances: module docstring of weight_families)."""
    case = wf.variant_case(family)
    assert np.isfinite(case["p32"]).all() and np.isfinite(case["l64"]).all()
    assert case["own"] <= 1e-5, (family, case["own"])
    assert np.abs(case["p64"].sum(1) - 1).max() < 1e-12
    # the probes begin with the int8 extremes
    assert (case["x"][0] == 127).all() and (case["x"][1] == -128).all() and (case["x"][2] == 0).all()


@pytest.mark.parametrize("shape", VARIANT_SHAPES[1:], ids=str)
def test_variant_shapes_stay_conditioned(shape):
    """confident_head keeps head x 12 at both shapes (two layers: 9.0e-6, 48 features x 21 rows: 3.7e-6)."""
    for family in ("default", "confident_head"):
        case = wf.variant_case(family, **shape)
        assert case["x"].shape[1:] == (shape.get("window", 33), shape.get("image_features", 26))
        assert case["own"] <= 1e-5, (family, shape, case["own"])
    if "image_features" in shape:           # the columns past V-syn's 26 are not left zero
        assert (wf.variant_case("default", **shape)["x"][3:, :, 26:] != 0).any()


def test_variant_confident_head_reaches_the_trained_regime():
    """All three classes called, logits past 10, a best probability above 0.9999 on one probe and below 0.5 on another
    (96 probes: a draw of 64 has 0.57 as its least confident call); the gain-1 default -- what every family test saw
    before -- calls at most two classes with every logit below 0.2."""
    case = wf.variant_case("confident_head", n_probes=96)
    best = case["p64"].max(axis=1)
    assert len(np.unique(case["p64"].argmax(1))) == 3
    assert np.abs(case["l64"]).max() > 10
    assert best.max() > 0.9999 and best.min() < 0.5
    # the 64 probes the GPU tests embed: all three classes as well, 0.57 to 0.99999
    best = wf.variant_case("confident_head")["p64"].max(axis=1)
    assert len(np.unique(wf.variant_case("confident_head")["p64"].argmax(1))) == 3 and best.max() > 0.9999 and best.min() < 0.6
    flat = wf.variant_case("default", n_probes=96)
    assert len(np.unique(flat["p64"].argmax(1))) <= 2 and np.abs(flat["l64"]).max() < 0.2


@pytest.mark.parametrize("terms", [3, 1])
@pytest.mark.parametrize("family", wf.HEAD_FAMILIES)
def test_head_families_make_a_missing_term_visible(family, terms):
    """The emulated product arithmetic (three terms) stays within 2e-5 of float64 on the head families; with the lo halves
    dropped (hi*hi only) it is at least 10 x the 1e-4 bar away -- on mixed_row_scales that error is 2.9e-6 and would pass."""
    case = wf.variant_case(family)
    n = 12
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pe, le = wf.variant_forward_emulated(case["sd"], case["x"][:n], terms=terms)
    err = max(wf.errors(pe, le, case["p64"][:n], case["l64"][:n]))
    if terms == 3:
        assert err < 2e-5, (family, err)
    else:
        assert err >= 10 * 1e-4, (family, err)


def test_variant_float64_restatement_is_pinned_by_the_reference_golden(golden_dir):
    """variant_forward_f64 against what the reference's own model class produced on the confident head (float32 torch;
    make_golden.py make_variant(head_scale=12)): within 2e-5, logits relative to their largest."""
    import os
    from pepper_amd import synthetic
    g = np.load(os.path.join(golden_dir, "variant_confident.npz"))
    sd = synthetic.variant_state_dict(seed=int(g["seed"]), gain=float(g["gain"]))
    sd["output_layer_type.weight"] *= np.float32(g["head_scale"])
    sd["output_layer_type.bias"] *= np.float32(g["head_scale"])
    assert g["images"].dtype == np.int8 and g["images"].shape == (64, 33, 26)
    assert np.abs(g["logits"]).max() > 10 and g["probs"].max() > 0.9999          # the fixture is in the confident regime
    p64, l64 = models_np.variant_forward_f64(sd, g["images"])
    assert max(wf.errors(g["probs"], g["logits"], p64, l64)) < 2e-5


# ---- polish families (tests/weight_families.py make_polish; GPU leg: tests/test_gpu_polish_stress.py) ----------------
POLISH_SHAPES = [{}, {"num_classes": 3}, {"num_classes": 7}, {"gru_layers": 2}]


def test_polish_float64_restatement_is_pinned_by_the_reference_goldens(golden_dir):
    """polish_predict_chunks_f64 against the accumulators the reference's own model class produced (float32 torch): the
    default recipe at gain 3 and the confident head."""
    import os
    from pepper_amd import synthetic
    for tag in ("g3", "confident"):
        g = np.load(os.path.join(golden_dir, f"polish_{tag}.npz"))
        sd = synthetic.polish_state_dict(seed=int(g["seed"]), gain=float(g["gain"]))
        if "head_scale" in g.files:
            sd["dense1.weight"] *= np.float32(g["head_scale"])
            sd["dense1.bias"] *= np.float32(g["head_scale"])
        acc64, counts = models_np.polish_predict_chunks_f64(sd, g["images"], 128)
        assert np.abs(acc64 - g["acc"]).max() < 2e-5, tag
        assert (counts[:, :50] == 1).all() and (counts[:, 950:] == 1).all() and (counts[:, 50:950] == 2).all()


@pytest.mark.parametrize("family", wf.POLISH_FAMILIES)
def test_polish_family_keeps_the_recurrence_conditioned(family):
    """A family is a parity case only while the float32 restatement itself stays within 1e-5 of float64 on the test's own
    chunks (measured distances: module docstring of weight_families)."""
    case = wf.polish_case(family)
    assert np.isfinite(case["acc32"]).all() and np.isfinite(case["acc64"]).all()
    assert case["own"] <= 1e-5, (family, case["own"])
    # each accumulated position is a sum of one or two softmax rows
    assert np.abs(case["acc64"].sum(2) - case["counts"]).max() < 1e-12


@pytest.mark.parametrize("shape", POLISH_SHAPES + [{"hidden": 256}], ids=str)
def test_polish_shapes_stay_conditioned(shape):
    n = 6 if shape.get("hidden") == 256 else wf.POLISH_CHUNKS
    for family in ("default", "confident_head"):
        assert wf.polish_case(family, n=n, **shape)["own"] <= 1e-5, (family, shape)


def test_confident_head_reaches_the_trained_regime():
    """phred 100 (t == 0 exactly) in the counts == 1 and in the counts == 2 region, and a spread of phred values between."""
    case = wf.polish_case("confident_head")
    edge = case["counts"] == 1
    for acc in (case["acc32"], case["acc64"].astype(np.float32)):
        _, phred, _, t = wf.polish_phred_from_acc(acc, case["counts"])
        assert (phred[t == 0] == 100).all() and (phred[t > 0] < 100).all()
        assert (t[edge] == 0).sum() > 100 and (t[~edge] == 0).sum() > 100
        assert len(np.unique(phred)) >= 40
    # a default-recipe head stays below phred 10: what every polish test saw before
    assert wf.polish_phred_from_acc(wf.polish_case("default")["acc32"], case["counts"])[1].max() < 10


def test_polish_near_tie_head_produces_near_ties():
    case = wf.polish_case("near_tie_head")
    top2 = np.sort(case["acc64"], axis=2)[:, :, -2:]
    gap = top2[:, :, 1] - top2[:, :, 0]
    assert gap.max() < 1e-3 and (gap > 0).all()
    assert len(np.unique(case["acc64"].argmax(2))) > 1          # and no class wins everywhere


@pytest.mark.parametrize("family", ["default"] + wf.POLISH_FAMILIES)
def test_finalize_restated_in_float64_agrees_with_the_float32_formula(family):
    """The expected phred of the GPU tests is floor(-10 log10(float64(t))) with t = f32(1 - f32(best / counts)); the
    restatement of predict_distributed_cpu.py:83-90 takes log10 in float32.  The two agree except where ph is within 1e-4
    of an integer, and such positions are at most 0.2 % of a call."""
    case = wf.polish_case(family)
    labels, phred, ph, t = wf.polish_phred_from_acc(case["acc32"], case["counts"])
    values = case["acc32"].max(axis=2)
    with np.errstate(divide="ignore"):
        ph32 = -10.0 * np.log10((1.0 - values / case["counts"].astype(np.float32)).astype(np.float32))
    ph32[np.isinf(ph32)] = 100
    excused = (t > 0) & (np.abs(ph - np.round(ph)) < 1e-4)
    assert excused.mean() <= 2e-3, excused.mean()
    assert ((phred == ph32.astype(np.uint8)) | excused).all()
    assert (labels == case["acc32"].argmax(2)).all()
