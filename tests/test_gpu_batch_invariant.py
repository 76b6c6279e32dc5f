"""Batch-invariant mode (pa_variant_set_batch_invariant / pa_polish_set_batch_invariant): with it on, a window's variant
probabilities and logits, and a chunk's polish labels, phred and accumulated softmax, are the same bits whatever the call
size, max_chunk, the row position and neighbours, the handle's earlier calls and the entry point.  The reference bits are
those of one full 16 384-window (chunk) call."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import models_np
from pepper_amd import _lib, synthetic
import weight_families

pytestmark = pytest.mark.gpu
TOL = 1e-4
BIG = 16384
SIZES = [1, 2, 63, 64, 65, 511, 512, 513, 1024, 1025, 3072, 3073, 16421]


class Variant:
    """Raw C-ABI harness: host and device int8 entry points, probabilities and logits of one call."""

    def __init__(self, sd, max_chunk=0, batch_invariant=True):
        self.lib = _lib.load()
        cfg = _lib.VariantConfig(26, 33, 1, 3, 0, max_chunk)
        names, data, numel, n, keep = _lib.marshal_state_dict(sd)
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.pa_variant_create(ctypes.byref(cfg), names, data, numel, n, None, ctypes.byref(self.h)))
        if batch_invariant:
            self.set(1)

    def set(self, on):
        _lib.check(self.lib.pa_variant_set_batch_invariant(self.h, int(on)))

    def get(self):
        v = ctypes.c_int32(-1)
        _lib.check(self.lib.pa_variant_get_batch_invariant(self.h, ctypes.byref(v)))
        return v.value

    def host(self, x):
        x = np.ascontiguousarray(x, dtype=np.int8)
        n = x.shape[0]
        probs, logits = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        _lib.check(self.lib.pa_variant_forward_host(self.h, x.ctypes.data, n, probs.ctypes.data, logits.ctypes.data))
        return probs, logits

    def device(self, x):
        xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.int8)).cuda()
        n = xd.shape[0]
        probs = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        logits = torch.empty_like(probs)
        torch.cuda.synchronize()
        _lib.check(self.lib.pa_variant_forward_device(self.h, xd.data_ptr(), n, probs.data_ptr(), logits.data_ptr()))
        _lib.check(self.lib.pa_synchronize(self.h))
        return probs.cpu().numpy(), logits.cpu().numpy()

    def overflow_rows(self):
        rows = ctypes.c_int64()
        _lib.check(self.lib.pa_variant_overflow_rows(self.h, ctypes.byref(rows)))
        return rows.value

    def close(self):
        if self.h:
            self.lib.pa_variant_destroy(self.h)
            self.h = None


def _embed(probes, n, rng, pool_seed):
    """A call of n windows: random neighbours with min(n, len(probes)) of the probes at random rows -> (x, rows, k)."""
    k = min(n, len(probes))
    x = synthetic.variant_windows(n, seed=pool_seed)
    rows = rng.choice(n, size=k, replace=False)
    x[rows] = probes[:k]
    return x, rows, k


def _check_variant_invariance(sd):
    rng = np.random.default_rng(11)
    probes = synthetic.variant_windows(64, seed=123)
    ref_handle = Variant(sd)
    x, rows, _ = _embed(probes, BIG, rng, pool_seed=7)
    p, l = ref_handle.host(x)
    ref_p, ref_l = p[rows], l[rows]
    assert np.isfinite(ref_p).all() and np.isfinite(ref_l).all()
    with np.errstate(over="ignore"):
        oracle_p, inter = models_np.variant_forward(sd, probes, return_intermediates=True)
    assert np.abs(ref_p - oracle_p).max() <= TOL
    assert np.abs(ref_l - inter["logits"]).max() <= TOL * max(1.0, float(np.abs(inter["logits"]).max()))
    # the same handle again, and handles of other pass sizes; one that ran a full call and then a 512 call first
    warmed = Variant(sd)
    warmed.host(synthetic.variant_windows(BIG, seed=8))
    warmed.host(synthetic.variant_windows(512, seed=9))
    handles = {"ref": ref_handle, "192": Variant(sd, max_chunk=192), "4096": Variant(sd, max_chunk=4096),
               "16384": Variant(sd, max_chunk=16384), "warmed": warmed}
    try:
        for n in SIZES:
            x, rows, k = _embed(probes, n, rng, pool_seed=1000 + n)
            for name, h in handles.items():
                for entry in ("host", "device"):
                    if name == "192" and entry == "device" and n > 4096:
                        continue        # (the host form covers this handle's many passes)
                    p, l = getattr(h, entry)(x)
                    assert np.array_equal(p[rows], ref_p[:k]), (n, name, entry)
                    assert np.array_equal(l[rows], ref_l[:k]), (n, name, entry)
    finally:
        for h in handles.values():
            h.close()


def test_variant_bits_do_not_depend_on_the_call():
    _check_variant_invariance(synthetic.variant_state_dict(gain=2.0))


@pytest.mark.parametrize("family", weight_families.FAMILIES)
def test_variant_bits_do_not_depend_on_the_call_weight_families(family):
    _check_variant_invariance(weight_families.make(family, seed=31))


def _mlp_peaks(sd, x):
    """Per window: the largest |activation| that enters or leaves linear_2 .. linear_5 (what the MLP kernel stores as h2)."""
    _, inter = models_np.variant_forward(sd, x, return_intermediates=True)
    a = inter["dec"].reshape(len(x), -1).astype(np.float64)
    peak = np.zeros(len(x))
    for name in ("linear_1", "linear_2", "linear_3", "linear_4", "linear_5"):
        a = models_np.selu(a @ sd[f"{name}.weight"].T.astype(np.float64) + sd[f"{name}.bias"])
        if name != "linear_5":
            peak = np.maximum(peak, np.abs(a).max(axis=1))
    return peak


def test_32_row_step_loops_give_the_64_row_bits(monkeypatch):
    """Up to small_rows windows the mode runs both step loops (the int8 first layer and the fused decoder) in 32-row
    workgroups; PA_SMALL_ROWS=0 keeps them at 64 rows.  Same bits, at every size the 32-row form takes."""
    sd = synthetic.variant_state_dict(gain=2.0)
    fast = Variant(sd)
    monkeypatch.setenv("PA_SMALL_ROWS", "0")
    wide = Variant(sd)
    monkeypatch.delenv("PA_SMALL_ROWS")
    try:
        for n in (1, 31, 32, 33, 100, 512, 1000, 1024, 3072):
            x = synthetic.variant_windows(n, seed=300 + n)
            a, b = fast.host(x), wide.host(x)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), n
    finally:
        fast.close()
        wide.close()


def test_one_overflowing_row_leaves_its_neighbours_bits_alone():
    """linear_2 .. linear_4 scaled so that some windows' activations pass 65504: a tile with exactly one such window.  The
    overflow counter rises by one, that row gets the f32 result, and the other 63 rows are the bits they have without it."""
    sd = synthetic.variant_state_dict(seed=5, gain=2.0)
    for name in ("linear_2", "linear_3", "linear_4"):
        sd[name + ".weight"] *= 38.0
    sd["linear_5.weight"] *= 1e-4
    pool = synthetic.variant_windows(2048, seed=21)
    with np.errstate(over="ignore"):
        peak = _mlp_peaks(sd, pool)
    # (the kernel's activations agree with these float64 ones to ~1e-6 relative: a 2 % margin on either side is ample)
    hot = np.flatnonzero(peak > 1.02 * 65504.0)
    cold = np.flatnonzero(peak < 0.9 * 65504.0)
    assert len(hot) >= 1 and len(cold) >= 64, (len(hot), len(cold))
    tile = pool[cold[:64]].copy()
    tile[17] = pool[hot[0]]
    clean = pool[cold[:64]]
    m = Variant(sd)
    try:
        before = m.overflow_rows()
        p, l = m.host(tile)
        assert m.overflow_rows() - before == 1
        p0, l0 = m.host(clean)
        assert m.overflow_rows() - before == 1
        others = np.arange(64) != 17
        assert np.array_equal(p[others], p0[others]) and np.array_equal(l[others], l0[others])
        with np.errstate(over="ignore"):
            ref = models_np.variant_forward(sd, tile[17:18])
        assert np.isfinite(p).all() and np.abs(p[17] - ref[0]).max() <= TOL
    finally:
        m.close()


def test_exact_f32_checkpoint_keeps_the_guarantee():
    """A checkpoint with weights beyond kSplitMaxWeight runs on the exact-f32 kernels; their schedule does not depend on the
    call, so the mode is accepted there and its bits are call-independent too."""
    sd = weight_families.make("near_f16_limit", seed=31)
    rng = np.random.default_rng(5)
    probes = synthetic.variant_windows(64, seed=124)
    a, b = Variant(sd), Variant(sd, max_chunk=192)
    try:
        assert a.get() == 1
        x, rows, _ = _embed(probes, 4096, rng, pool_seed=70)
        ref_p, ref_l = a.host(x)
        ref_p, ref_l = ref_p[rows], ref_l[rows]
        assert np.isfinite(ref_p).all()
        for n in (1, 64, 513, 3073):
            x, rows, k = _embed(probes, n, rng, pool_seed=80 + n)
            for h in (a, b):
                for entry in ("host", "device"):
                    p, l = getattr(h, entry)(x)
                    assert np.array_equal(p[rows], ref_p[:k]) and np.array_equal(l[rows], ref_l[:k]), (n, entry)
    finally:
        a.close()
        b.close()


def test_the_switch_is_a_real_switch():
    sd = synthetic.variant_state_dict(gain=2.0)
    x = synthetic.variant_windows(512, seed=55)
    on_ref = Variant(sd)
    off_ref = Variant(sd, batch_invariant=False)
    m = Variant(sd, batch_invariant=False)
    try:
        assert off_ref.get() == 0 and on_ref.get() == 1
        p_on, l_on = on_ref.host(x)
        p_off, l_off = off_ref.host(x)
        assert not (np.array_equal(p_on, p_off) and np.array_equal(l_on, l_off)), "the mode changes nothing at n = 512"
        for _ in range(2):
            m.set(1)
            assert m.get() == 1
            p, l = m.host(x)
            assert np.array_equal(p, p_on) and np.array_equal(l, l_on)
            m.set(0)
            assert m.get() == 0
            p, l = m.host(x)
            assert np.array_equal(p, p_off) and np.array_equal(l, l_off)
    finally:
        for h in (on_ref, off_ref, m):
            h.close()


# ---------------------------------------------------------------------------------------------------------------------
# polish
# ---------------------------------------------------------------------------------------------------------------------
POLISH_SIZES = [1, 17, 128, 4096, 4097, 16384, 16400]


class Polish:
    def __init__(self, sd, max_chunk=0, batch_invariant=True):
        self.lib = _lib.load()
        cfg = _lib.PolishConfig(10, 128, 1, 5, 1000, 100, 50, 50, 0, max_chunk)
        names, data, numel, n, keep = _lib.marshal_state_dict(sd)
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.pa_polish_create(ctypes.byref(cfg), names, data, numel, n, None, ctypes.byref(self.h)))
        if batch_invariant:
            _lib.check(self.lib.pa_polish_set_batch_invariant(self.h, 1))

    def host(self, x):
        x = np.ascontiguousarray(x, dtype=np.uint8)
        n = x.shape[0]
        lab, ph = np.empty((n, 1000), np.uint8), np.empty((n, 1000), np.uint8)
        acc = np.empty((n, 1000, 5), np.float32)
        _lib.check(self.lib.pa_polish_predict_host(self.h, x.ctypes.data, n, lab.ctypes.data, ph.ctypes.data,
                                                   acc.ctypes.data))
        return lab, ph, acc

    def parts(self, x, k, rng):
        n = x.shape[0]
        cuts = np.sort(rng.choice(np.arange(1, n), size=min(k - 1, n - 1), replace=False)) if n > 1 else np.array([], int)
        bounds = [0] + cuts.tolist() + [n]
        imgs = [np.ascontiguousarray(x[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
        labs = [np.empty((len(i), 1000), np.uint8) for i in imgs]
        phs = [np.empty((len(i), 1000), np.uint8) for i in imgs]
        P = ctypes.c_void_p * len(imgs)
        counts = (ctypes.c_int64 * len(imgs))(*[len(i) for i in imgs])
        _lib.check(self.lib.pa_polish_predict_host_parts(self.h, len(imgs), P(*[i.ctypes.data for i in imgs]), counts,
                                                         P(*[a.ctypes.data for a in labs]), P(*[a.ctypes.data for a in phs])))
        return np.concatenate(labs), np.concatenate(phs)

    def close(self):
        if self.h:
            self.lib.pa_polish_destroy(self.h)
            self.h = None


def _check_polish_invariance(sd, sizes, small_sizes, big=BIG, oracle=True):
    """Probes inside one call of `big` chunks are the reference; then every size through the same handle (host and host
    parts), a max_chunk = 192 handle (host, the sizes in small_sizes) and a handle that ran a larger call first."""
    rng = np.random.default_rng(3)
    probes = synthetic.polish_chunks(32, seed=66)
    m, small = Polish(sd), Polish(sd, max_chunk=192)
    warmed = Polish(sd)
    try:
        x = synthetic.polish_chunks(big, seed=67)
        rows = rng.choice(big, size=32, replace=False)
        x[rows] = probes
        lab, ph, acc = m.host(x)
        ref_lab, ref_ph, ref_acc = lab[rows], ph[rows], acc[rows]
        assert np.isfinite(ref_acc).all()
        if oracle:
            rl, rp, inter = models_np.polish_predict_chunks(sd, probes[:4], 128, return_intermediates=True)
            assert np.abs(ref_acc[:4] - inter["acc"]).max() <= TOL
        warmed.host(synthetic.polish_chunks(big, seed=68))
        for n in sizes:
            k = min(n, 32)
            x = synthetic.polish_chunks(n, seed=500 + n)
            rows = rng.choice(n, size=k, replace=False)
            x[rows] = probes[:k]
            for name, h in (("ref", m), ("warmed", warmed)) + ((("192", small),) if n in small_sizes else ()):
                lab, ph, acc = h.host(x)
                assert np.array_equal(lab[rows], ref_lab[:k]) and np.array_equal(ph[rows], ref_ph[:k]), (n, name)
                assert np.array_equal(acc[rows], ref_acc[:k]), (n, name)
            for parts in (1, 3, 7):
                lab, ph = m.parts(x, parts, rng)
                assert np.array_equal(lab[rows], ref_lab[:k]) and np.array_equal(ph[rows], ref_ph[:k]), (n, parts)
    finally:
        for h in (m, small, warmed):
            h.close()


def test_polish_bits_do_not_depend_on_the_call():
    _check_polish_invariance(synthetic.polish_state_dict(seed=5, gain=2.0), POLISH_SIZES, (1, 17, 128, 4097, 16400))


def test_polish_exact_f32_checkpoint_refuses_the_mode():
    """Polish weights beyond kSplitMaxWeight select the exact-f32 GRU kernels, and those were measured to give a chunk
    different labels at different call sizes: turning the mode on there fails with PA_ERR_UNSUPPORTED, says why, and leaves
    the handle as it was; the Python wrapper raises rather than run without the guarantee."""
    from pepper_amd.polish.models.simple_model import TransducerGRU as PolishModel
    sd = synthetic.polish_state_dict(seed=5, gain=2.0)
    rng = np.random.default_rng(8)
    for k, v in sd.items():
        if v.ndim == 2 and "gru" in k:
            hit = rng.random(v.shape) < 5e-4
            v[hit] = rng.choice([-200.0, 200.0], size=int(hit.sum())).astype(np.float32)
    m = Polish(sd, batch_invariant=False)
    try:
        assert m.lib.pa_polish_set_batch_invariant(m.h, 1) == _lib.PA_ERR_UNSUPPORTED
        assert b"exact-f32" in m.lib.pa_last_error()
        v = ctypes.c_int32(-1)
        _lib.check(m.lib.pa_polish_get_batch_invariant(m.h, ctypes.byref(v)))
        assert v.value == 0
        _lib.check(m.lib.pa_polish_set_batch_invariant(m.h, 0))          # turning it off is always accepted
        lab, ph, acc = m.host(synthetic.polish_chunks(3, seed=4))
        assert np.isfinite(acc).all()
    finally:
        m.close()
    with pytest.raises(_lib.PepperAmdError) as e:
        PolishModel(1, 10, 1, 128, 5, batch_invariant=True).load_state_dict(sd)
    assert e.value.code == _lib.PA_ERR_UNSUPPORTED


def test_polish_switch_toggles():
    sd = synthetic.polish_state_dict(seed=5, gain=2.0)
    x = synthetic.polish_chunks(128, seed=12)
    on_ref, off_ref, m = Polish(sd), Polish(sd, batch_invariant=False), Polish(sd, batch_invariant=False)
    try:
        want_on, want_off = on_ref.host(x), off_ref.host(x)
        assert not np.array_equal(want_on[2], want_off[2]), "the mode changes nothing at 128 chunks"
        for _ in range(2):
            for on, want in ((1, want_on), (0, want_off)):
                _lib.check(m.lib.pa_polish_set_batch_invariant(m.h, on))
                v = ctypes.c_int32(-1)
                _lib.check(m.lib.pa_polish_get_batch_invariant(m.h, ctypes.byref(v)))
                assert v.value == on
                got = m.host(x)
                assert all(np.array_equal(g, w) for g, w in zip(got, want)), on
    finally:
        for h in (on_ref, off_ref, m):
            h.close()


def test_polish_switch_and_wrapper():
    """The Python wrapper turns the mode on from its argument and reads it back; a small call in the mode equals the same
    chunks inside a full-sized call."""
    from pepper_amd.polish.models.simple_model import TransducerGRU as PolishModel
    sd = synthetic.polish_state_dict(seed=5, gain=2.0)
    pm = PolishModel(1, 10, 1, 128, 5, batch_invariant=True).load_state_dict(sd)
    off = PolishModel(1, 10, 1, 128, 5).load_state_dict(sd)
    try:
        assert pm.get_batch_invariant() and not off.get_batch_invariant()
        x = synthetic.polish_chunks(4096, seed=9)
        big = np.concatenate([x, synthetic.polish_chunks(BIG - 4096, seed=10)])
        lab_big, ph_big = pm.predict_chunks(torch.from_numpy(big))
        lab, ph = pm.predict_chunks(torch.from_numpy(x))
        assert np.array_equal(lab.numpy(), lab_big.numpy()[:4096]) and np.array_equal(ph.numpy(), ph_big.numpy()[:4096])
        clone = pm.clone()
        assert clone.get_batch_invariant()
        clone.close()
    finally:
        pm.close()
        off.close()
