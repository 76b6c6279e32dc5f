"""linear_1's split-K GEMM on 16x16x32 MFMAs (gemm_h2.hip: gemm_h2_k32_kernel), through pa_debug_gemm_h2_split: the same host
operands, one h2 conversion, the split-K slices once by the new kernel and once by the parent's gemm_h2_kernel<0>, both
through splitk_finish_kernel.

1. Against float64 numpy on the h2-rounded operands (hi + lo as float64), at the edges of the 16-row MFMA tile, the 128-row
   wave tile, the 256-row workgroup tile and a ragged last workgroup (a_rows = M: the row clamp is exercised), N = 512 and a
   ragged column tile (N = 96), slices of one k-tile (the prologue requests its only tile three times), odd slice lengths
   (LDS stage parity) and uneven slices (5 k-tiles over 2 slices: 2 and 3; 66 over 32: 2 and 3 mixed), with and without SELU
   in the finish.  The parent kernel's largest error is measured in the same test on the same operands; the new kernel's may
   be at most twice that (both add the same f32 products, in another order inside an instruction), 0 where the parent's is
   0, and every output is finite.
2. Values near 6e4 with an all-zero A row and an all-zero W row.
3. Slice independence: rows 0..32 of an M = 33 call equal the same rows of an M = 513 call bit for bit.
4. The whole variant model against the float64 oracle at n in {1, 17, 129, 257} on default-scale and gain-2 weights (1e-4),
   and batch-invariant mode: a 33-window call and the first 33 rows of a 3073-window call give equal bits."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import models_np
from pepper_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

F = ctypes.POINTER(ctypes.c_float)
ROWS = [1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 513]
SLICES = [(2, 2), (3, 2), (5, 2), (5, 4), (66, 32)]          # (K / 32, splits)
TOL = 1e-4


def run_split(A, W, bias, M, N, act, splits, iters=1):
    """(C of the new kernel, C of the parent kernel, ms new, ms parent)."""
    lib = _lib.load()
    fn = lib.pa_debug_gemm_h2_split
    fn.restype = ctypes.c_int
    fn.argtypes = [F, F, F, F, F] + [ctypes.c_int] * 7 + [F, F]
    A = np.ascontiguousarray(A[:M], np.float32)
    W = np.ascontiguousarray(W, np.float32)
    C_new, C_par = np.full((M, N), np.nan, np.float32), np.full((M, N), np.nan, np.float32)
    ms_new, ms_par = ctypes.c_float(), ctypes.c_float()
    bp = bias.ctypes.data_as(F) if bias is not None else None
    rc = fn(A.ctypes.data_as(F), W.ctypes.data_as(F), bp, C_new.ctypes.data_as(F), C_par.ctypes.data_as(F), M, M, N, A.shape[1],
            act, splits, iters, ctypes.byref(ms_new), ctypes.byref(ms_par))
    assert rc == 0, _lib.last_error()
    return C_new, C_par, ms_new.value, ms_par.value


def h2_rounded(x):
    """What the kernels multiply: hi = f16(v), lo = f16(v - hi), as float64 hi + lo."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64) + lo.astype(np.float64)


def selu(x):
    return 1.0507009873554805 * np.where(x > 0, x, 1.6732632423543772 * np.expm1(x))


@functools.lru_cache(maxsize=None)
def operands(N, K):
    """Normal(0, 1) operands of the largest call (the smaller calls take its first rows) and their float64 product + bias."""
    rng = np.random.default_rng(1000 * N + K)
    A = rng.standard_normal((max(ROWS), K)).astype(np.float32)
    W = rng.standard_normal((N, K)).astype(np.float32)
    bias = rng.uniform(-0.5, 0.5, size=N).astype(np.float32)
    ref = h2_rounded(A) @ h2_rounded(W).T + bias.astype(np.float64)
    for arr in (A, W, bias, ref):
        arr.setflags(write=False)
    return A, W, bias, ref


def check(C_new, C_par, ref, what):
    assert np.isfinite(C_new).all() and np.isfinite(C_par).all(), what
    err_new, err_par = float(np.abs(C_new - ref).max()), float(np.abs(C_par - ref).max())
    print(f"{what}: max |C - C64|  new {err_new:.3g}  parent {err_par:.3g}")
    if err_par == 0.0:
        assert err_new == 0.0, what
    assert err_new <= 2.0 * err_par, (what, err_new, err_par)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("ktiles,splits", SLICES)
@pytest.mark.parametrize("N", [512, 96])
def test_against_float64_and_the_parent_kernel(N, ktiles, splits, act):
    A, W, bias, ref = operands(N, 32 * ktiles)
    if act:
        ref = selu(ref)
    for M in ROWS:
        C_new, C_par, _, _ = run_split(A, W, bias, M, N, act, splits)
        check(C_new, C_par, ref[:M], f"M={M} N={N} K={32 * ktiles} splits={splits} act={act}")


def test_large_values_and_zero_rows():
    rng = np.random.default_rng(11)
    M, N, K = 257, 256, 256
    A = (rng.uniform(5.9e4, 6.1e4, size=(M, K)) * rng.choice([-1.0, 1.0], size=(M, K))).astype(np.float32)
    W = (rng.uniform(5.9e4, 6.1e4, size=(N, K)) * rng.choice([-1.0, 1.0], size=(N, K))).astype(np.float32)
    A[3, :] = 0
    W[5, :] = 0
    ref = h2_rounded(A) @ h2_rounded(W).T
    for splits in (2, 4):
        C_new, C_par, _, _ = run_split(A, W, None, M, N, 0, splits)
        check(C_new, C_par, ref, f"large values, splits={splits}")
        assert not C_new[3].any() and not C_new[:, 5].any()


def test_a_rows_chain_does_not_depend_on_the_call_size():
    A, W, bias, _ = operands(512, 32 * 66)
    small = run_split(A, W, bias, 33, 512, 0, 32)[0]
    big = run_split(A, W, bias, 513, 512, 0, 32)[0]
    assert np.array_equal(small, big[:33])


# ---- the whole model

SIZES = [1, 17, 129, 257]
FAMILIES = {"default-scale": dict(seed=5, gain=1.0), "gain-2": dict(seed=5, gain=2.0)}


class Model:
    """Raw C-ABI harness around one variant model."""

    def __init__(self, sd, batch_invariant=False):
        self.lib = _lib.load()
        cfg = _lib.VariantConfig(26, 33, 1, 3, 0, 0)
        names, data, numel, n, keep = _lib.marshal_state_dict(sd)
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.pa_variant_create(ctypes.byref(cfg), names, data, numel, n, None, ctypes.byref(self.h)))
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


@pytest.fixture(scope="module")
def model_results():
    """Per family: the oracle's probabilities of one pool of windows (computed once) and the model's, from calls of SIZES."""
    pool = synthetic.variant_windows(sum(SIZES), seed=621)
    starts = np.cumsum([0] + SIZES[:-1])
    where = {n: slice(int(s), int(s) + n) for n, s in zip(SIZES, starts)}
    out = {}
    for family, kw in FAMILIES.items():
        sd = synthetic.variant_state_dict(**kw)
        with np.errstate(over="ignore"):
            oracle = models_np.variant_forward_f64(sd, pool)[0]
        m = Model(sd)
        p = np.empty((len(pool), 3), np.float32)
        for n in SIZES:
            p[where[n]] = m.forward(pool[where[n]])[0]
        m.close()
        out[family] = (oracle, p, where)
    return out


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("n", SIZES)
def test_model_against_the_float64_oracle(model_results, family, n):
    oracle, got, where = model_results[family]
    err = float(np.abs(got[where[n]] - oracle[where[n]]).max())
    print(f"oracle  {family:13s} n={n:3d}  max |p - p64| = {err:.3g}")
    assert np.isfinite(got[where[n]]).all()
    assert err <= TOL


def test_model_batch_invariant_bits():
    sd = synthetic.variant_state_dict(seed=5, gain=2.0)
    x = synthetic.variant_windows(3073, seed=622)
    m = Model(sd, batch_invariant=True)
    p_small, l_small = m.forward(x[:33])
    p_big, l_big = m.forward(x)
    m.close()
    assert np.isfinite(p_big).all()
    assert np.array_equal(p_small, p_big[:33]) and np.array_equal(l_small, l_big[:33])
