"""The polish model where trained checkpoints live: confident heads, stress families of weights, the model shapes
pa_polish_create accepts, the large-weight fallback -- every head form against the float64 restatement
(oracle/models_np.py polish_predict_chunks_f64), and polish_finalize_kernel exactly.

Families: tests/weight_families.py make_polish; 20 chunks (one 16-row slab of polish_combine_kernel and one 16-row
small-call tile crossed, a ragged end in the 128-row tile and the 256-row head block), one chunk zero from position 300.

Head forms (environment read at model creation):
  small-call   the default: gru_small_h2 + polish_dense_acc_h2_kernel
  big-fused    PA_POLISH_SMALL_MAX=0: gru_dec_h2 with dense1 inside the step loop + polish_combine_kernel
  big-split    PA_POLISH_SMALL_MAX=0 PA_FUSE_HEAD=0: gru_dec_h2 + polish_dense_acc_h2_kernel
  f32-loops    PA_SPLIT_REC=0: the f32 step loops + polish_dense_acc_kernel<256>
Hidden size 256 takes the f32 loops and polish_dense_acc_kernel<512> whatever the environment; 6 to 8 classes take
dense_small_kernel<1> in every form.

MEASURED (MI355X) max |acc - acc64|, beside the float32 numpy restatement's own distance from float64 on the same chunks;
`excused` is the largest share of positions per call whose phred was excused because -10 log10(t) lies within 1e-4 of an
integer (bound: 0.2 %):

    family, shape            small-call big-fused  big-split  f32-loops  f32 numpy  excused
    default, h128            2.07e-07   4.84e-07   4.48e-07   2.03e-07   1.47e-07   0.005 %
    graded_head, h128        2.70e-06   6.13e-06   6.25e-06   2.65e-06   1.24e-06   0.005 %
    confident_head, h128     8.17e-06   1.75e-05   1.72e-05   8.29e-06   4.10e-06   0.015 %
    near_tie_head, h128      7.02e-08   2.36e-07   6.90e-08   6.65e-08   7.87e-08   0.000 %
    mixed_row_scales, h128   2.08e-07   2.19e-06   2.19e-06   2.61e-07   1.52e-07   0.000 %
    large_bias, h128         2.77e-07   4.91e-07   5.35e-07   2.72e-07   2.11e-07   0.005 %
    large_entries, h128      2.45e-06   1.17e-05   1.17e-05   1.73e-06   1.94e-06   0.000 %
    default, c3              2.84e-07   5.92e-07   5.59e-07   2.58e-07   1.99e-07   0.025 %
    confident_head, c3       8.10e-06   1.73e-05   1.73e-05   8.24e-06   4.36e-06   0.005 %
    default, c7              1.50e-07   3.37e-07   3.37e-07   1.42e-07   1.11e-07   0.060 %
    confident_head, c7       8.95e-06   2.19e-05   2.19e-05   8.23e-06   3.77e-06   0.035 %
    default, l2              1.79e-07   2.42e-07   2.41e-07   1.41e-07   1.17e-07   0.000 %
    confident_head, l2       6.64e-06   9.82e-06   9.99e-06   5.68e-06   2.50e-06   0.030 %
    default, h256            2.14e-07   -          -          -          1.42e-07   0.017 %
    confident_head, h256     6.98e-06   -          -          -          4.17e-06   0.000 %
    one weight of 3e4 / 7e4  6.69e-06 / 6.72e-06 (the f32 kernels)       1.42e-05 / 1.37e-05
The bar is 0.5e-4 (1e-4 for the large-weight fallback).  The big-call step loops (K = 384 contraction, projection inside
the loop) sit 2 to 10 times further from float64 than the small-call ones, the largest 2.2e-5 on the confident head.
Golden of the reference's model class (polish_confident.npz): acc distance 5.5e-6 / 1.3e-5 / 1.4e-5 / 5.8e-6 in the four
forms, 0 phred mismatches on the 1599 judged positions in each.

Each finalize behaviour was also broken on purpose once (clamp to 99, `p <= overlap`, last maximum wins, rounding cast, a
cap at 60): test_finalize_is_exact failed for every one of them, the golden test for all but the label rule.
"""
import os

import numpy as np
import pytest
import torch

import weight_families as wf
from oracle import models_np
from pepper_amd import synthetic

pytestmark = pytest.mark.gpu
TOL = 1e-4
ENV_KEYS = ("PA_POLISH_SMALL_MAX", "PA_FUSE_HEAD", "PA_SPLIT_REC", "PA_SPLIT_GEMM")
FORMS = {"small-call": {}, "big-fused": {"PA_POLISH_SMALL_MAX": "0"},
         "big-split": {"PA_POLISH_SMALL_MAX": "0", "PA_FUSE_HEAD": "0"}, "f32-loops": {"PA_SPLIT_REC": "0"}}
SHAPES = {"h128": {}, "h256": {"hidden": 256}, "c3": {"num_classes": 3}, "c7": {"num_classes": 7}, "l2": {"gru_layers": 2}}

CASES = [(family, "h128", form) for family in ["default"] + wf.POLISH_FAMILIES for form in FORMS]
# shapes nothing else builds; hidden size 256 has one form (its step loops are the f32 ones)
CASES += [(family, shape, form) for shape in ("c3", "c7", "l2") for family in ("default", "confident_head") for form in FORMS]
CASES += [(family, "h256", "small-call") for family in ("default", "confident_head")]
IDS = ["-".join(c) for c in CASES]


@pytest.fixture(scope="module")
def oracle():
    """(family, shape) -> the case of weight_families.polish_case: weights, chunks, float64 accumulator, counts, and the
    float32 restatement's own distance; computed once per family and shape."""
    def get(family, shape):
        return wf.polish_case(family, n=6 if shape == "h256" else wf.POLISH_CHUNKS, **SHAPES[shape])
    return get


def _predict(sd, x, form, hidden=128, num_classes=5, gru_layers=1):
    """One predict_chunks call under a head form -> dict(labels, phred, acc, prof) as numpy / the set of kernel labels."""
    from pepper_amd import _lib
    from pepper_amd.polish.models.simple_model import TransducerGRU
    saved = {k: os.environ.get(k) for k in ENV_KEYS}
    try:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(FORMS[form])
        m = TransducerGRU(1, 10, gru_layers, hidden, num_classes, bidirectional=True).load_state_dict(sd)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        _lib.check(_lib.load().pa_profile_enable(m.handle, 1))
        labels, phred, acc = m.predict_chunks(torch.from_numpy(x).cuda(), return_acc=True)
        prof = set(_lib.profile_dict(m.handle))
    finally:
        m.close()
    return dict(labels=labels.cpu().numpy(), phred=phred.cpu().numpy(), acc=acc.cpu().numpy(), prof=prof)


_RUNS = {}


def _run(oracle, family, shape, form):
    key = (family, shape, form)
    if key not in _RUNS:
        case = oracle(family, shape)
        _RUNS[key] = _predict(case["sd"], case["x"], form, **SHAPES[shape])
    return _RUNS[key]


def _check_kernel_labels(prof, form, hidden=128, num_classes=5):
    """The form really ran its kernels (labels of api.hip's LAUNCH_TRY)."""
    h2_loops = {k for k in prof if k.startswith("gru_") and "_h2" in k}
    assert "polish_finalize" in prof, prof
    if hidden == 256 or form == "f32-loops":
        assert "gru_rec" in prof and "dense_softmax_acc" in prof and not h2_loops and "head_combine_acc" not in prof, prof
        assert "cvt_f32" not in prof, prof
        return
    if form == "small-call":
        assert "gru_small_h2" in prof and h2_loops == {"gru_small_h2"} and "dense_softmax_acc" in prof, prof
    elif form == "big-fused" and num_classes <= 5:
        assert {"gru_rec_h2_fused_in", "gru_dec_h2_fused_dense", "head_combine_acc"} <= prof, prof
        assert "dense_softmax_acc" not in prof and "gru_small_h2" not in prof, prof
    else:
        assert {"gru_rec_h2_fused_in", "gru_dec_h2_fused", "dense_softmax_acc"} <= prof, prof
        assert "head_combine_acc" not in prof and "gru_dec_h2_fused_dense" not in prof and "gru_small_h2" not in prof, prof
    # more than 5 classes: the h2 layer output is converted back for dense_small_kernel<1>
    assert ("cvt_f32" in prof) == (num_classes > 5), prof


def _check_acc(acc, case, bar, what):
    acc64 = case["acc64"]
    assert acc.shape == acc64.shape and np.isfinite(acc).all(), what
    dist = float(np.abs(acc - acc64).max())
    print(f"MEASURED {'-'.join(what)}: gpu {dist:.2e}  f32 restatement {case['own']:.2e}")
    assert dist < bar, (what, dist, case["own"])
    top2 = np.sort(acc64, axis=2)[:, :, -2:]
    clear = (top2[:, :, 1] - top2[:, :, 0]) > 2 * TOL
    assert (acc.argmax(2)[clear] == acc64.argmax(2)[clear]).all(), what


def _phred_as_judged(acc, counts):
    """Expected phred from the device's own accumulator under given counts, int16; -1 where 1 - best / counts < 0 (no
    such position exists under the right counts)."""
    _, phred, ph, t = wf.polish_phred_from_acc(acc, counts)
    return np.where(t < 0, -1, phred.astype(np.int16)), ph, t


def _check_finalize(run, counts, what, overlap=50, flat=False):
    """labels / phred of one call against polish_finalize_kernel's four behaviours, recomputed on the host from the call's
    own f32 accumulator: first-maximum-wins labels, the cast of -10 log10(1 - best / counts), the clamp to 100 where that
    is infinite, counts 1 on the first and last `overlap` columns and 2 between.  flat: a head whose best class stays near
    1 / C reads phred 0 under either count on the outer columns, nothing to tell there.  -> share of excused positions."""
    acc, labels, phred = run["acc"], run["labels"], run["phred"]
    S = acc.shape[1]
    want_labels, want, ph, t = wf.polish_phred_from_acc(acc, counts)
    assert (t >= 0).all(), what
    assert labels.dtype == np.uint8 and phred.dtype == np.uint8
    assert (labels == want_labels).all(), what
    # device log10f against the host's float64 log10: an ulp apart moves floor() only where ph is all but an integer
    excused = (t > 0) & (np.abs(ph - np.round(ph)) < 1e-4)
    share = float(excused.mean())
    assert share <= 2e-3, (what, share)
    ok = (phred == want) | (excused & ((phred == np.floor(ph - 0.5)) | (phred == np.floor(ph + 0.5))))
    assert ok.all(), (what, int((~ok).sum()), phred[~ok][:8], want[~ok][:8], t[~ok][:8])
    assert (phred[t == 0] == 100).all(), what                       # never excused
    assert (phred[t > 0] < 100).all(), what                         # f32 t > 0 is at least 2^-24: phred <= 72
    # the boundary: judged under the other count, these columns would read differently
    other = np.where(counts == 1, 2.0, 1.0)
    wrong, _, _ = _phred_as_judged(acc, other)
    for cols, n_counts in ((slice(0, overlap), 1), (slice(S - overlap, S), 1), (slice(overlap, overlap + 1), 2),
                           (slice(S - overlap - 1, S - overlap), 2)):
        assert (counts[:, cols] == n_counts).all()
        tells = (wrong[:, cols] != want[:, cols]) & ~excused[:, cols]
        assert tells.any() or (flat and n_counts == 1), (what, cols)
        assert (phred[:, cols][tells] == want[:, cols][tells]).all(), (what, cols)
    return share


@pytest.mark.parametrize("family,shape,form", CASES, ids=IDS)
def test_accumulator_against_float64(oracle, family, shape, form):
    """max |acc - acc64| < 0.5 * TOL in every head form, finite, labels equal wherever float64 separates the two best
    classes by more than 2 * TOL; and the form ran the kernels it is named for."""
    case = oracle(family, shape)
    assert case["own"] <= 1e-5, case["own"]            # a parity case: the recurrence stays conditioned (checked on the CPU too)
    run = _run(oracle, family, shape, form)
    kw = SHAPES[shape]
    _check_kernel_labels(run["prof"], form, kw.get("hidden", 128), kw.get("num_classes", 5))
    _check_acc(run["acc"], case, 0.5 * TOL, (family, shape, form))
    if family == "near_tie_head":
        top2 = np.sort(run["acc"], axis=2)[:, :, -2:]
        assert (top2[:, :, 1] - top2[:, :, 0]).max() < 1e-3


@pytest.mark.parametrize("family,shape,form", CASES, ids=IDS)
def test_finalize_is_exact(oracle, family, shape, form):
    case = oracle(family, shape)
    run = _run(oracle, family, shape, form)
    share = _check_finalize(run, case["counts"], (family, shape, form), flat=family == "near_tie_head")
    print(f"EXCUSED {family}-{shape}-{form}: {100 * share:.3f} %")
    edge = case["counts"] == 1
    hundred = run["phred"] == 100
    if family == "confident_head" and shape != "l2":
        # (two GRU layers at this seed: the float64 oracle's largest phred is 72, no position saturates)
        assert hundred[edge].any() and hundred[~edge].any()
        assert len(np.unique(run["phred"])) >= 40
    if family == "near_tie_head":
        # first maximum wins: the accumulator holds exact ties of the best class, and the lowest index is the label
        best = run["acc"].max(axis=2, keepdims=True)
        assert ((run["acc"] == best).sum(axis=2) > 1).any()
    # saturation where exact arithmetic saturates: float64 best / counts within 2^-26 of 1 rounds to t == 0 in any f32 head
    sure = (1.0 - case["acc64"].max(2) / case["counts"]) < 2.0 ** -27
    assert hundred[sure].all()


def test_large_weights_run_the_f32_kernels_and_meet_the_bar(oracle):
    """A GRU weight of 64 or more (api.hip kSplitMaxWeight) sends the checkpoint to the exact-f32 kernels: no _h2 kernel
    label, acc within TOL of float64 (the float32 restatement is 1.4e-5 away itself), finalize exact."""
    x = oracle("default", "h128")["x"]
    for big in (3.0e4, 7.0e4):
        sd = synthetic.polish_state_dict(seed=3)
        sd["gru_decoder.weight_hh_l0"][2 * 128 + 5, 7] = big       # 7e4 would not even fit the f16 hi half
        acc64, counts = models_np.polish_predict_chunks_f64(sd, x, 128)
        _, _, inter = models_np.polish_predict_chunks(sd, x, 128, return_intermediates=True)
        case = dict(acc64=acc64, counts=counts, own=float(np.abs(inter["acc"] - acc64).max()))
        run = _predict(sd, x, "small-call")
        assert not any("_h2" in k for k in run["prof"]), (big, run["prof"])
        assert "gru_rec" in run["prof"] and "dense_softmax_acc" in run["prof"], run["prof"]
        _check_acc(run["acc"], case, TOL, ("large_weight", f"{big:g}", "fallback"))
        _check_finalize(run, counts, ("large_weight", big))


def test_confident_head_matches_the_reference_golden(golden_dir):
    """tests/golden/polish_confident.npz: the reference's own model class and window loop on the confident head (make_golden.py
    make_polish(head_scale=40)) -- its inf -> 100 replacement and its uint8 cast in the regime where they act."""
    g = np.load(os.path.join(golden_dir, "polish_confident.npz"))
    sd = synthetic.polish_state_dict(seed=int(g["seed"]), gain=float(g["gain"]))
    sd["dense1.weight"] *= np.float32(g["head_scale"])
    sd["dense1.bias"] *= np.float32(g["head_scale"])
    assert (g["phred"] == 100).sum() > 50 and len(np.unique(g["phred"])) >= 40      # the fixture is in that regime
    pf = g["phred_f32"]
    frac = pf - np.floor(pf)
    judged = (pf < 60) & (frac > 5e-2) & (frac < 1 - 5e-2)
    counts = np.full(pf.shape, 2.0)
    counts[:, :50] = counts[:, 950:] = 1.0
    for form in FORMS:
        run = _predict(sd, g["images"], form)
        dist = float(np.abs(run["acc"] - g["acc"]).max())
        miss = int((run["phred"][judged] != g["phred"][judged]).sum())
        print(f"GOLDEN {form}: acc distance {dist:.2e}, phred mismatches on judged positions {miss} of {int(judged.sum())}")
        assert dist < TOL, form
        assert miss == 0, (form, miss)
        _, _, _, t = wf.polish_phred_from_acc(run["acc"], counts)
        at = (g["phred"] == 100) & (t == 0)
        assert at.sum() > 50 and (run["phred"][at] == 100).all(), form
        top2 = np.sort(g["acc"], axis=2)[:, :, -2:]
        clear = (top2[:, :, 1] - top2[:, :, 0]) > 2 * TOL
        assert (run["labels"] == g["labels"])[clear].all(), form
