// The weight layout of the fused LSTM step loops on v_mfma_f32_16x16x32_f16 (rnn_h2.hip: lstm_dec_h2_body, KX = 2H, and
// lstm_enc_h2_body, the int8 first layer, KX = 32), which contract [h | x] with [W_hh | W_ih]: where a weight's f16 hi and
// lo halves live, and the host packer that puts them there (api.hip build_rec_layer, for these layers only: every other
// step loop keeps pack_rec_weights_h2).  Plain inline functions, no HIP types and no _Float16: g++ and hipcc both compile
// this file.
//
//     [dir][gate][column tile of 16][k step of 32][hi, lo][64 lanes][16 B]
//     lane l of (gate g, column tile c, k step s) holds W[g*H + 16c + (l & 15)][32s + 8(l >> 4) + e], e = 0..7
//
// W = [W_hh | W_ih] is [4H, K] per direction, K = H + KX; the B operand of the instruction wants, per lane, eight consecutive
// k of one output column (gru_small_h2_kernel and the DENSE head use the same operand layout).  Same bytes as
// pack_rec_weights_h2.  Any number of k steps: K = H + KX must be a multiple of 32.
// A first layer with F < KX input features keeps W_ih in columns [H, H + F), zeros beyond, and -- when a bias is given --
// bias[d][n] in column H + F: the step loop feeds a constant 1.0 in that input column, so the matrix pipe adds the bias
// (pack_rec_weights_h2's bias column).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace pa_dec16 {

// float -> IEEE binary16, round to nearest even (what a (_Float16) conversion gives); beyond the f16 range -> infinity
inline uint16_t f16_bits(float v) {
    uint32_t x;
    memcpy(&x, &v, 4);
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(sign | (x > 0x7f800000u ? 0x7e00u : 0x7c00u));
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);           // >= 65520 rounds to infinity
    if (x < 0x38800000u) {                                              // below 2^-14: a subnormal half, round(|v| * 2^24)
        if (x <= 0x33000000u) return sign;                              // <= 2^-25 rounds (ties) to zero
        const int shift = 126 - (int)(x >> 23);                         // 14 .. 24
        const uint32_t m = (x & 0x7fffffu) | 0x800000u;
        uint32_t r = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
        if (rem > half || (rem == half && (r & 1u))) ++r;
        return (uint16_t)(sign | r);
    }
    const uint32_t r = x - 0x38000000u;                                 // exponent bias 127 -> 15
    uint32_t m = r >> 13;
    const uint32_t rem = r & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (m & 1u))) ++m;            // a carry out of the mantissa lands in the exponent
    return (uint16_t)(sign | m);
}

inline float f16_value(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    uint32_t x;
    if (e == 31u) x = sign | 0x7f800000u | (m << 13);
    else if (e != 0u) x = sign | ((e + 112u) << 23) | (m << 13);
    else if (m == 0u) x = sign;
    else {
        float f = (float)m * (1.0f / 16777216.0f);                      // m * 2^-24, exact
        memcpy(&x, &f, 4);
        x |= sign;
    }
    float f;
    memcpy(&f, &x, 4);
    return f;
}

// 32-bit words of both directions' fragments
inline size_t words(int H, int KX) { return (size_t)2 * 4 * (H / 16) * ((H + KX) / 32) * 2 * 256; }

// index, in f16 halves, of element e of lane l of fragment (dir d, gate g, column tile c, k step s, half hl: 0 hi, 1 lo)
inline size_t half_index(int H, int KX, int d, int g, int c, int s, int hl, int l, int e) {
    return ((((((size_t)d * 4 + g) * (H / 16) + c) * ((H + KX) / 32) + s) * 2 + hl) * 64 + l) * 8 + e;
}

// whh[d]: [4H, H], wih[d]: [4H, F] (row n = g*H + unit), both row-major f32 -> out[words(H, KX)].  F < 0: F = KX.
// bias (may be null): bias[d][4H], placed in column H + F when F < KX.
inline void pack(const float* const whh[2], const float* const wih[2], int H, int KX, uint32_t* out, int F = -1,
                 const float* const* bias = nullptr) {
    if (F < 0) F = KX;
    uint16_t* o = reinterpret_cast<uint16_t*>(out);
    const int KS = (H + KX) / 32, CT = H / 16;
    for (int d = 0; d < 2; ++d)
        for (int g = 0; g < 4; ++g)
            for (int c = 0; c < CT; ++c)
                for (int s = 0; s < KS; ++s)
                    for (int l = 0; l < 64; ++l)
                        for (int e = 0; e < 8; ++e) {
                            const int n = g * H + 16 * c + (l & 15), k = 32 * s + 8 * (l >> 4) + e;
                            float v = 0.0f;
                            if (k < H) v = whh[d][(size_t)n * H + k];
                            else if (k - H < F) v = wih[d][(size_t)n * F + (k - H)];
                            else if (bias != nullptr && k - H == F && F < KX) v = bias[d][n];
                            const uint16_t hi = f16_bits(v);
                            o[half_index(H, KX, d, g, c, s, 0, l, e)] = hi;
                            o[half_index(H, KX, d, g, c, s, 1, l, e)] = f16_bits(v - f16_value(hi));
                        }
}

}  // namespace pa_dec16
