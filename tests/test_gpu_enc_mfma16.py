"""The fused int8 LSTM encoder on 16x16x32 MFMAs (rnn_h2.hip lstm_enc_h2_kernel, weights in the order of csrc/dec_frag16.h with the
bias column).

Every model here is created with PA_UNIT_SPLIT=0 and PA_SMALL_BATCH=0: the first layer of an int8 call is the fused encoder at
every call size, and the decoder behind it is the same fused kernel in every model of this file.  PA_SMALL_ROWS=0 keeps the
encoder on 64-row workgroups; batch-invariant mode with the default PA_SMALL_ROWS runs it on 32-row workgroups.

1. Probabilities against the float64 oracle at the edges of the 16-row tiles, of the 32- and 64-row workgroups and of a ragged
   last workgroup, on default-scale and on gain-2 weights, for the 64-row form and (batch-invariant mode) the 32-row form,
   held to the project's 1e-4.
   Largest error measured (MI355X), parent commit (32x32x16 encoder) -> this kernel:
       default-scale  64-row 8.85e-08 -> 8.67e-08   32-row 8.59e-08 -> 9.03e-08
       gain-2         64-row 1.15e-06 -> 1.20e-06   32-row 1.60e-06 -> 1.59e-06
2. Against the unfused path: the same windows as f32 through the device entry point, whose first layer is the projection GEMM
   and the unchanged step loop seeded from Xp (lstm_seed_h2_kernel, 32x32x16 tiles).  The parent's fused encoder
   differs from that path by 5.96e-08 (default-scale) and 8.94e-07 (gain-2) on these inputs (largest probability
   difference); twice that is allowed.  Measured with this kernel: 5.96e-08 and 8.94e-07.
3. Batch-invariant mode: a 33-window call (32-row workgroups) and the first 33 rows of a 3073-window call (64-row workgroups)
   give equal bits.
4. Both directions and the int8 extremes: windows that differ only at t = 0, and windows that differ only at t = 32, two of
   them by features of -128 and 127; what the difference does to the probabilities matches the oracle within 1e-4
   (measured: effect error 1.5e-06 at most, on effects of 0.08-0.14; the parent: 1.5e-06).
5. The instantiation without the bias column (BC = false) is the one a model of 32 image features selects: such a model
   against the oracle on 64-row workgroups (the 32-row launch of such a model has no fused form).  Measured: 6.2e-08 (the
   parent: 5.5e-08)."""
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
# twice what the parent commit's fused encoder differs from its unfused path by on inputs() below (docstring, 2)
SEEDED_TOL = {"default-scale": 2 * 5.96e-08, "gain-2": 2 * 8.94e-07}


class Model:
    """Raw C-ABI harness; the schedule switches are read at creation."""

    def __init__(self, sd, small_rows=None, batch_invariant=False, features=26):
        env = {"PA_SMALL_BATCH": "0", "PA_UNIT_SPLIT": "0"}
        if small_rows is not None:
            env["PA_SMALL_ROWS"] = str(small_rows)
        saved = {k: os.environ.get(k) for k in list(env) + ["PA_SMALL_ROWS"]}
        os.environ.pop("PA_SMALL_ROWS", None)
        os.environ.update(env)
        try:
            self.lib = _lib.load()
            cfg = _lib.VariantConfig(features, 33, 1, 3, 0, 0)
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

    def forward_unfused(self, x):
        """The same windows as f32 on the device: the first layer runs as projection GEMM + the step loop seeded from Xp."""
        import torch
        xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
        n = x.shape[0]
        probs, logits = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        _lib.check(self.lib.pa_variant_forward_device_f32(self.h, xd.data_ptr(), n, probs.data_ptr(), logits.data_ptr()))
        _lib.check(self.lib.pa_synchronize(self.h))
        torch.cuda.synchronize()
        return probs.cpu().numpy(), logits.cpu().numpy()

    def close(self):
        self.lib.pa_variant_destroy(self.h)


def inputs():
    """One pool of windows; the call of size n takes the n windows after those of the smaller sizes."""
    pool = synthetic.variant_windows(sum(SIZES), seed=711)
    starts = np.cumsum([0] + SIZES[:-1])
    return pool, {n: slice(int(s), int(s) + n) for n, s in zip(SIZES, starts)}


@pytest.fixture(scope="module")
def results():
    """Per family: the oracle's probabilities of the pool (computed once), and those of the 64-row fused encoder, the 32-row
    fused encoder (batch-invariant mode) and the unfused path, each from calls of the sizes of SIZES."""
    pool, where = inputs()
    out = {}
    for family, kw in FAMILIES.items():
        sd = synthetic.variant_state_dict(**kw)
        with np.errstate(over="ignore"):
            oracle = models_np.variant_forward_f64(sd, pool)[0]
        got = {}
        for form, (small_rows, bi, unfused) in {"fused-64": (0, False, False), "fused-32": (None, True, False),
                                                "unfused": (0, False, True)}.items():
            m = Model(sd, small_rows, batch_invariant=bi)
            p = np.empty((len(pool), 3), np.float32)
            for n in SIZES:
                p[where[n]] = (m.forward_unfused if unfused else m.forward)(pool[where[n]])[0]
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
def test_against_the_unfused_path(results, family):
    oracle, got, _ = results[family]
    assert np.abs(got["unfused"] - oracle).max() <= TOL          # the unfused path is the model too
    diff = np.abs(got["fused-64"].astype(np.float64) - got["unfused"].astype(np.float64)).max(axis=1)
    print(f"unfused {family:13s} max |p_fused - p_unfused| = {diff.max():.3g}  (allowed {SEEDED_TOL[family]:.3g})")
    assert diff.max() <= SEEDED_TOL[family]


def test_batch_invariant_bits_of_the_32_and_the_64_row_form():
    sd = synthetic.variant_state_dict(seed=5, gain=2.0)
    x = synthetic.variant_windows(3073, seed=712)
    m = Model(sd, batch_invariant=True)
    p_small, l_small = m.forward(x[:33])
    p_big, l_big = m.forward(x)
    m.close()
    assert np.isfinite(p_big).all()
    assert np.array_equal(p_small, p_big[:33]) and np.array_equal(l_small, l_big[:33])


@pytest.mark.parametrize("t_diff", [0, 32])
def test_both_directions_and_the_int8_extremes(t_diff):
    """40 windows equal to one base window except at time step t_diff: the forward direction carries a difference at t = 0
    through all 33 steps, the reverse direction one at t = 32.  Windows 1 and 2 differ from the base by features of -128 and
    127 as well."""
    sd = synthetic.variant_state_dict(seed=5, gain=2.0)
    pool = synthetic.variant_windows(41, seed=713)
    x = np.repeat(pool[:1], 40, axis=0)
    x[1:, t_diff] = pool[1:40, t_diff]
    x[1, t_diff, 3], x[1, t_diff, 25] = -128, 127
    x[2, t_diff, 0], x[2, t_diff, 12] = 127, -128
    assert x.dtype == np.int8 and x.min() == -128 and x.max() == 127
    with np.errstate(over="ignore"):
        oracle = models_np.variant_forward_f64(sd, x)[0]
    effect = oracle[1:] - oracle[:1]
    assert np.abs(effect).max() > 10 * TOL          # the inputs do tell the windows apart (an oracle-side fact)
    for small_rows, bi in ((0, False), (None, True)):
        m = Model(sd, small_rows, batch_invariant=bi)
        p = m.forward(x)[0].astype(np.float64)
        m.close()
        err, eff_err = np.abs(p - oracle).max(), np.abs((p[1:] - p[:1]) - effect).max()
        print(f"directions t={t_diff:2d} batch_invariant={bi}: max |p - p64| = {err:.3g}, effect error {eff_err:.3g}, "
              f"largest effect {np.abs(effect).max():.3g}")
        assert err <= TOL and eff_err <= TOL


def test_the_form_without_the_bias_column():
    """32 image features leave no input column for the bias: lstm_enc_h2_kernel<2, false> adds the four
    biases in the gate phase.  (The 32-row launch of a 32-feature model has no fused form and is not reached here.)"""
    sd = synthetic.variant_state_dict(seed=7, gain=1.0, image_features=32)
    rng = np.random.default_rng(714)
    x = rng.integers(-12, 13, (65, 33, 32)).astype(np.int8)
    x[3, 5, 31], x[4, 6, 0] = -128, 127
    with np.errstate(over="ignore"):
        oracle = models_np.variant_forward_f64(sd, x)[0]
    m = Model(sd, 0, features=32)
    p = m.forward(x)[0]
    m.close()
    err = float(np.abs(p - oracle).max())
    print(f"no bias column: max |p - p64| = {err:.3g}")
    assert np.isfinite(p).all() and err <= TOL
