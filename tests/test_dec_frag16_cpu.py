"""The fused LSTM decoder's weight layout (pepper_amd/csrc/dec_frag16.h) without a GPU: the header compiled by the host compiler
into a stand-alone program, with AddressSanitizer and UBSan, packs a seeded [1024, 768] matrix per direction; every f16 half it
writes is compared with a NumPy restatement of the layout

    [dir][gate][column tile of 16][k step of 32][hi, lo][64 lanes][16 B]
    lane l of (gate g, column tile c, k step s) holds W[g*256 + 16c + (l & 15)][32s + 8(l >> 4) + e], e = 0..7

and hi + lo must give the f32 weight back to 2^-22 relative.

That bound is what the two f16 halves can carry, where they can carry it: hi is off by at most 2^-11 |v|, the remainder
r = v - hi is exact in f32, and lo is off by at most 2^-11 |r| <= 2^-22 |v| while r is a normal f16 (|r| >= 2^-14), by at most
2^-25 (half a subnormal step) otherwise -- which is still <= 2^-22 |v| for |v| >= 2^-3.  So the bulk of the matrix is drawn with
2^-3 <= |v| < 8 and held to the relative bound; a band of rows holds what the conversion itself can get wrong (zeros, signed
values down to below the smallest subnormal half, exact rounding ties, the largest finite half) and is held to
max(2^-22 |v|, 2^-25) -- and to the bit-for-bit comparison like everything else."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, KX = 256, 512
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
    if (argc != 4) return 2;
    const int H = 256, KX = 512;
    const std::vector<float> whh = slurp(argv[1], (size_t)2 * 4 * H * H), wih = slurp(argv[2], (size_t)2 * 4 * H * KX);
    const float* const whh_d[2] = {whh.data(), whh.data() + (size_t)4 * H * H};
    const float* const wih_d[2] = {wih.data(), wih.data() + (size_t)4 * H * KX};
    std::vector<uint32_t> out(pa_dec16::words(H, KX));      // exactly as many as the packer may write: ASan watches the ends
    pa_dec16::pack(whh_d, wih_d, H, KX, out.data());
    FILE* f = fopen(argv[3], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    fclose(f);
    printf("%zu\n", out.size());
    return 0;
}
"""


def seeded_weights():
    rng = np.random.default_rng(20260)
    w = rng.uniform(0.125, 8.0, (2, 4 * H, K)).astype(np.float32)
    w = np.where(w >= 8.0, np.float32(7.5), w) * rng.choice(np.float32([-1.0, 1.0]), w.shape)
    # rows 40-47 of both directions: what the conversion itself can get wrong
    edge = np.float32([0.0, -0.0, 65504.0, -65504.0, 2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, -(2.0 ** -26),
                       1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -22, 2047.5 * 2.0 ** -24, 2.0 ** -14 - 2.0 ** -26,
                       1e-3, -3e-5, 6e-8, 1 / 3, 0.1])
    band = np.resize(edge, (2, 8, K)) * np.resize(np.float32([1, -1, 1]), (2, 8, K))
    band[:, 4:] = rng.uniform(-0.125, 0.125, (2, 4, K)).astype(np.float32) * np.float32(2.0) ** rng.integers(-14, 1, (2, 4, K)).astype(np.float32)
    w[:, 40:48] = band
    return np.ascontiguousarray(w, np.float32)


def restated_layout(w):
    """-> uint16 [dir][gate][column tile][k step][hi, lo][lane][e]"""
    hi = w.astype(np.float16)
    lo = (w - hi.astype(np.float32)).astype(np.float16)
    d, g, c, s, l, e = np.meshgrid(np.arange(2), np.arange(4), np.arange(H // 16), np.arange(K // 32), np.arange(64), np.arange(8),
                                   indexing="ij")
    n, k = g * H + 16 * c + (l & 15), 32 * s + 8 * (l >> 4) + e
    return np.stack([hi[d, n, k], lo[d, n, k]], axis=4).view(np.uint16)


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dec_frag16")
    src, exe = tmp / "pack_main.cpp", tmp / "pack_main"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "pepper_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    w = seeded_weights()
    np.ascontiguousarray(w[:, :, :H]).tofile(tmp / "whh.f32")
    np.ascontiguousarray(w[:, :, H:]).tofile(tmp / "wih.f32")
    run = subprocess.run([str(exe), str(tmp / "whh.f32"), str(tmp / "wih.f32"), str(tmp / "out.u32")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert int(run.stdout) == 2 * 4 * (H // 16) * (K // 32) * 2 * 256
    return w, np.fromfile(tmp / "out.u32", np.uint16).reshape(2, 4, H // 16, K // 32, 2, 64, 8)


def test_every_half_sits_where_the_layout_says(packed):
    w, got = packed
    want = restated_layout(w)
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_hi_plus_lo_gives_the_weight_back(packed):
    w, got = packed
    halves = got.view(np.float16).astype(np.float64)
    d, g, c, s, l, e = np.meshgrid(np.arange(2), np.arange(4), np.arange(H // 16), np.arange(K // 32), np.arange(64), np.arange(8),
                                   indexing="ij")
    n, k = g * H + 16 * c + (l & 15), 32 * s + 8 * (l >> 4) + e
    v = w.astype(np.float64)[d, n, k]
    err = np.abs(halves[:, :, :, :, 0] + halves[:, :, :, :, 1] - v)
    big = np.abs(v) >= 0.125
    assert big.mean() > 0.99
    print("largest relative error where |v| >= 2^-3: %.3g x 2^-22" % ((err[big] / np.abs(v[big])).max() * 2.0 ** 22))
    assert (err[big] <= 2.0 ** -22 * np.abs(v[big])).all()
    assert (err[~big] <= np.maximum(2.0 ** -22 * np.abs(v[~big]), 2.0 ** -25)).all()
    # every (dir, row, k) of the matrix is held exactly once
    seen = np.zeros((2, 4 * H, K), np.int32)
    np.add.at(seen, (d.ravel(), n.ravel(), k.ravel()), 1)
    assert (seen == 1).all()
