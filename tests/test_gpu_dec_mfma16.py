"""The fused LSTM decoder on 16x16x32 MFMAs (rnn_h2.hip lstm_dec_h2_kernel, weights in the order of csrc/dec_frag16.h).

Every model here is created with PA_SMALL_BATCH=0, so the decoder layer runs the fused step loop at every call size, and with
PA_UNIT_SPLIT=0, so the encoder in front of it is the same kernel in every model of this file.

1. Probabilities against the float64 oracle at the edges of the 16-row tiles, of the 32- and 64-row workgroups and of a ragged
   last workgroup, on default-scale and on gain-2 weights, for the 64-row form and (batch-invariant mode) the 32-row form,
   held to the project's 1e-4.
   Largest error measured (MI355X), parent commit (32x32x16 decoder) -> this kernel:
       default-scale  64-row 9.19e-08 -> 7.59e-08   32-row 9.48e-08 -> 8.89e-08
       gain-2         64-row 1.38e-06 -> 1.33e-06   32-row 1.85e-06 -> 1.85e-06
2. Against the unchanged decoder seeded from Xp (lstm_seed_h2_kernel, selected by a large PA_SMALL_BATCH): the same
   three-term arithmetic on 32x32x16 tiles.  The parent's fused form differs from the seeded form by 5.96e-08 (default-scale)
   and 1.19e-06 (gain-2) on these inputs (largest probability difference); twice that is allowed -- only the summation order
   inside an instruction changed.  Measured with this kernel: 5.96e-08 and 1.01e-06.
3. Batch-invariant mode: a 33-window call (32-row workgroups) and the first 33 rows of a 3073-window call (64-row workgroups)
   give equal bits.
4. Both directions: windows that differ only at t = 0, and windows that differ only at t = 32; what the difference does to
   the probabilities matches the oracle within the bar of 1 (measured: 1.4e-06 at most, on effects of 0.02-0.03)."""
import ctypes
import os

import numpy as np
import pytest

from oracle import models_np
from pepper_amd import _lib, synthetic

pytestmark = pytest.mark.gpu
TOL = 1e-4
SIZES = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129]
FAMILIES = {"default-scale": dict(seed=5, gain=1.0), "gain-2": dict(seed=5, gain=2.0)}
# twice what the parent commit's fused decoder differs from its seeded decoder by on inputs() below (docstring, 2)
SEEDED_TOL = {"default-scale": 2 * 5.96e-08, "gain-2": 2 * 1.19e-06}


class Model:
    """Raw C-ABI harness; the schedule switches are read at creation."""

    def __init__(self, sd, small_batch, batch_invariant=False):
        env = {"PA_SMALL_BATCH": str(small_batch), "PA_UNIT_SPLIT": "0"}
        saved = {k: os.environ.get(k) for k in list(env) + ["PA_SMALL_ROWS"]}
        os.environ.update(env)
        os.environ.pop("PA_SMALL_ROWS", None)
        try:
            self.lib = _lib.load()
            cfg = _lib.VariantConfig(26, 33, 1, 3, 0, 0)
            names, data, numel, n, keep = _lib.marshal_state_dict(sd)
            self.h = ctypes.c_void_p()
            _lib.check(self.lib.pa_variant_create(ctypes.byref(cfg), names, data, numel, n, None, ctypes.byref(self.h)))
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        if batch_invariant:
            _lib.check(self.lib.pa_variant_set_batch_invariant(self.h, 1))

    def forward(self, x):
        x = np.ascontiguousarray(x, dtype=np.int8)
        n = x.shape[0]
        probs, logits = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        _lib.check(self.lib.pa_variant_forward_host(self.h, x.ctypes.data, n, probs.ctypes.data, logits.ctypes.data))
        return probs, logits

    def close(self):
        self.lib.pa_variant_destroy(self.h)


def inputs():
    """One pool of windows; the call of size n takes the n windows after those of the smaller sizes."""
    pool = synthetic.variant_windows(sum(SIZES), seed=611)
    starts = np.cumsum([0] + SIZES[:-1])
    return pool, {n: slice(int(s), int(s) + n) for n, s in zip(SIZES, starts)}


@pytest.fixture(scope="module")
def results():
    """Per family: the oracle's probabilities of the pool (computed once), and those of the 64-row fused decoder, the 32-row
    fused decoder (batch-invariant mode) and the seeded decoder, each from calls of the sizes of SIZES."""
    pool, where = inputs()
    out = {}
    for family, kw in FAMILIES.items():
        sd = synthetic.variant_state_dict(**kw)
        with np.errstate(over="ignore"):
            oracle = models_np.variant_forward_f64(sd, pool)[0]
        got = {}
        for form, (small_batch, bi) in {"fused-64": (0, False), "fused-32": (0, True), "seeded": (1 << 20, False)}.items():
            m = Model(sd, small_batch, batch_invariant=bi)
            p = np.empty((len(pool), 3), np.float32)
            for n in SIZES:
                p[where[n]] = m.forward(pool[where[n]])[0]
            m.close()
            got[form] = p
        out[family] = (oracle, got, where)
    return out


@pytest.mark.parametrize("form", ["fused-64", "fused-32"])
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("n", SIZES)
def test_against_the_float64_oracle(results, family, form, n):
    oracle, got, where = results[family]
    err = float(np.abs(got[form][where[n]] - oracle[where[n]]).max())
    print(f"oracle  {family:13s} {form} n={n:3d}  max |p - p64| = {err:.3g}")
    assert np.isfinite(got[form][where[n]]).all()
    assert err <= TOL


@pytest.mark.parametrize("family", list(FAMILIES))
def test_against_the_seeded_decoder(results, family):
    _, got, _ = results[family]
    diff = np.abs(got["fused-64"].astype(np.float64) - got["seeded"].astype(np.float64)).max(axis=1)
    print(f"seeded  {family:13s} max |p_fused - p_seeded| = {diff.max():.3g}  (allowed {SEEDED_TOL[family]:.3g})")
    assert diff.max() <= SEEDED_TOL[family]


def test_batch_invariant_bits_of_the_32_and_the_64_row_form():
    sd = synthetic.variant_state_dict(seed=5, gain=2.0)
    x = synthetic.variant_windows(3073, seed=612)
    m = Model(sd, 0, batch_invariant=True)
    p_small, l_small = m.forward(x[:33])
    p_big, l_big = m.forward(x)
    m.close()
    assert np.isfinite(p_big).all()
    assert np.array_equal(p_small, p_big[:33]) and np.array_equal(l_small, l_big[:33])


@pytest.mark.parametrize("t_diff", [0, 32])
def test_both_directions(t_diff):
    """40 windows equal to one base window except at time step t_diff: the forward direction carries a difference at t = 0
    through all 33 steps, the reverse direction one at t = 32."""
    sd = synthetic.variant_state_dict(seed=5, gain=2.0)
    pool = synthetic.variant_windows(41, seed=613)
    x = np.repeat(pool[:1], 40, axis=0)
    x[1:, t_diff] = pool[1:40, t_diff]
    with np.errstate(over="ignore"):
        oracle = models_np.variant_forward_f64(sd, x)[0]
    effect = oracle[1:] - oracle[:1]
    assert np.abs(effect).max() > 10 * TOL          # the inputs do tell the windows apart (an oracle-side fact)
    for bi in (False, True):
        m = Model(sd, 0, batch_invariant=bi)
        p = m.forward(x)[0].astype(np.float64)
        m.close()
        err, eff_err = np.abs(p - oracle).max(), np.abs((p[1:] - p[:1]) - effect).max()
        print(f"directions t={t_diff:2d} batch_invariant={bi}: max |p - p64| = {err:.3g}, effect error {eff_err:.3g}, "
              f"largest effect {np.abs(effect).max():.3g}")
        assert err <= TOL and eff_err <= TOL
