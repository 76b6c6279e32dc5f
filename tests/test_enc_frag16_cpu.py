"""The fused int8 LSTM encoder's weight layout (pepper_amd/csrc/dec_frag16.h with nine k steps and the bias column) without a
GPU: the header compiled by the host compiler into a stand-alone program, with AddressSanitizer and UBSan, packs a seeded
[1024, 256] recurrent matrix, a [1024, 26] input matrix and a bias per direction into [1024, 288] x 2; every f16 half it writes
is compared with a NumPy restatement of the layout

    [dir][gate][column tile of 16][k step of 32][hi, lo][64 lanes][16 B]
    lane l of (gate g, column tile c, k step s) holds W[g*256 + 16c + (l & 15)][32s + 8(l >> 4) + e], e = 0..7
    W = [W_hh | W_ih (F columns) | bias (column H + F) | zeros]

and hi + lo must give the f32 value back to 2^-22 relative (tests/test_dec_frag16_cpu.py derives that bound: it holds for
|v| >= 2^-3, which is where the matrix is drawn from; the exact zeros of the padding must come back as zeros)."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, F, KX = 256, 26, 32
K = H + KX

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "dec_frag16.h"
static std::vector<float> slurp(const char* path, size_t n) {
    std::vector<float> v(n);
    FILE* f = fopen(path, "rb");
    if (!f || fread(v.data(), 4, n, f) != n) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fclose(f);
    return v;
}
int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const int H = 256, F = 26, KX = 32;
    // exactly as many values as the packer may read: ASan watches the ends of the F-wide rows and of the bias
    const std::vector<float> whh = slurp(argv[1], (size_t)2 * 4 * H * H), wih = slurp(argv[2], (size_t)2 * 4 * H * F),
                             bias = slurp(argv[3], (size_t)2 * 4 * H);
    const float* const whh_d[2] = {whh.data(), whh.data() + (size_t)4 * H * H};
    const float* const wih_d[2] = {wih.data(), wih.data() + (size_t)4 * H * F};
    const float* const bias_d[2] = {bias.data(), bias.data() + (size_t)4 * H};
    std::vector<uint32_t> out(pa_dec16::words(H, KX), 0xffffffffu);      // exactly as many as the packer may write
    pa_dec16::pack(whh_d, wih_d, H, KX, out.data(), F, bias_d);
    FILE* f = fopen(argv[4], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    fclose(f);
    printf("%zu\n", out.size());
    return 0;
}
"""


def seeded_matrix():
    """-> (w [2, 1024, 288] as the layout sees it, whh, wih, bias)"""
    rng = np.random.default_rng(20261)
    def draw(shape):
        v = rng.uniform(0.125, 8.0, shape).astype(np.float32)
        return np.where(v >= 8.0, np.float32(7.5), v) * rng.choice(np.float32([-1.0, 1.0]), shape)
    whh, wih, bias = draw((2, 4 * H, H)), draw((2, 4 * H, F)), draw((2, 4 * H))
    w = np.zeros((2, 4 * H, K), np.float32)
    w[:, :, :H], w[:, :, H:H + F], w[:, :, H + F] = whh, wih, bias
    return w, whh, wih, bias


def indices():
    d, g, c, s, l, e = np.meshgrid(np.arange(2), np.arange(4), np.arange(H // 16), np.arange(K // 32), np.arange(64), np.arange(8),
                                   indexing="ij")
    return d, g * H + 16 * c + (l & 15), 32 * s + 8 * (l >> 4) + e


def restated_layout(w):
    """-> uint16 [dir][gate][column tile][k step][hi, lo][lane][e]"""
    hi = w.astype(np.float16)
    lo = (w - hi.astype(np.float32)).astype(np.float16)
    d, n, k = indices()
    return np.stack([hi[d, n, k], lo[d, n, k]], axis=4).view(np.uint16)


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("enc_frag16")
    src, exe = tmp / "pack_main.cpp", tmp / "pack_main"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "pepper_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    w, whh, wih, bias = seeded_matrix()
    for name, v in (("whh", whh), ("wih", wih), ("bias", bias)):
        np.ascontiguousarray(v, np.float32).tofile(tmp / f"{name}.f32")
    run = subprocess.run([str(exe), str(tmp / "whh.f32"), str(tmp / "wih.f32"), str(tmp / "bias.f32"), str(tmp / "out.u32")],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert int(run.stdout) == 2 * 4 * (H // 16) * (K // 32) * 2 * 256
    return w, bias, np.fromfile(tmp / "out.u32", np.uint16).reshape(2, 4, H // 16, K // 32, 2, 64, 8)


def test_every_half_sits_where_the_layout_says(packed):
    w, _, got = packed
    want = restated_layout(w)
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_hi_plus_lo_gives_the_value_back(packed):
    w, _, got = packed
    halves = got.view(np.float16).astype(np.float64)
    d, n, k = indices()
    v = w.astype(np.float64)[d, n, k]
    err = np.abs(halves[:, :, :, :, 0] + halves[:, :, :, :, 1] - v)
    filled = k <= H + F
    assert (np.abs(v[filled]) >= 0.125).all()
    print("largest relative error: %.3g x 2^-22" % ((err[filled] / np.abs(v[filled])).max() * 2.0 ** 22))
    assert (err[filled] <= 2.0 ** -22 * np.abs(v[filled])).all()
    assert (got[:, :, :, :, :, :, :][np.broadcast_to(~filled[:, :, :, :, None], got.shape[:4] + (2,) + got.shape[5:])] == 0).all()
    # every (dir, row, k) of the matrix is held exactly once
    seen = np.zeros((2, 4 * H, K), np.int32)
    np.add.at(seen, (d.ravel(), n.ravel(), k.ravel()), 1)
    assert (seen == 1).all()


def test_the_bias_column_lands_at_k_equal_h_plus_f(packed):
    _, bias, got = packed
    s, q, e = (H + F) // 32, ((H + F) % 32) // 8, (H + F) % 8
    halves = got.view(np.float16).astype(np.float32)
    for d in range(2):
        for n in range(4 * H):
            g, c, l = n // H, (n % H) // 16, (n % 16) + 16 * q
            hi, lo = halves[d, g, c, s, 0, l, e], halves[d, g, c, s, 1, l, e]
            assert hi == np.float32(np.float16(bias[d, n])) and abs(float(hi) + float(lo) - float(bias[d, n])) <= 2.0 ** -22 * abs(bias[d, n])
