// The reservoir sample of an interval's reads, written once for the host (bamio.cpp: pa_reservoir_sample) and the device
// (encoder.hip: reservoir_keep_kernel).  Plain inline functions, no HIP types: g++ and hipcc both compile this file.
//
// What it restates (pepper_amd/variant/AlignmentSummarizer.py:49-57, the loop of the reference's utils.reservoir_sample):
//     random = numpy.random.RandomState(seed)
//     for i in range(n):
//         if len(sample) < k: sample.append(i)
//         else:
//             j = random.randint(0, i + 1)
//             if j < k: sample[j] = i
// numpy's legacy generator is MT19937 seeded by init_genrand; randint(0, i + 1) of the legacy stream draws nothing for
// i == 0 and otherwise takes 32-bit words `& mask` (mask = the smallest 2^b - 1 >= i) until one is <= i.  NumPy freezes that
// stream by policy (NEP 19).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PA_RS_FN __host__ __device__ inline
#else
#define PA_RS_FN inline
#endif

enum { PA_MT_N = 624, PA_MT_M = 397 };
// the three data-parallel stretches of a regeneration: words [0, 227) read old words only, [227, 454) read the new words of
// the first stretch, [454, 623) those of the second; word 623 reads the new word 0
enum { PA_MT_S1 = PA_MT_N - PA_MT_M, PA_MT_S2 = 2 * (PA_MT_N - PA_MT_M), PA_MT_S3 = PA_MT_N - 1 };

// word p of the key of legacy RandomState(seed), given word p - 1 (word 0 is the seed itself)
PA_RS_FN uint32_t pa_mt_seed_next(uint32_t prev, uint32_t p) { return 1812433253u * (prev ^ (prev >> 30)) + p; }

PA_RS_FN void pa_mt_seed(uint32_t* mt, uint32_t seed) {
    mt[0] = seed;
    for (uint32_t p = 1; p < PA_MT_N; ++p) mt[p] = pa_mt_seed_next(mt[p - 1], p);
}

// the new word kk of a regeneration: cur = mt[kk], next = mt[kk + 1] (mt[0] for the last word), far = mt[(kk + 397) % 624]
PA_RS_FN uint32_t pa_mt_twist_word(uint32_t cur, uint32_t next, uint32_t far) {
    const uint32_t y = (cur & 0x80000000u) | (next & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// where word kk of a regeneration reads its `far` word
PA_RS_FN int pa_mt_far(int kk) { return kk < PA_MT_S1 ? kk + PA_MT_M : kk - PA_MT_S1; }

PA_RS_FN void pa_mt_twist(uint32_t* mt) {
    for (int kk = 0; kk < PA_MT_N - 1; ++kk) mt[kk] = pa_mt_twist_word(mt[kk], mt[kk + 1], mt[pa_mt_far(kk)]);
    mt[PA_MT_N - 1] = pa_mt_twist_word(mt[PA_MT_N - 1], mt[0], mt[PA_MT_M - 1]);
}

PA_RS_FN uint32_t pa_mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// the smallest 2^b - 1 >= i
PA_RS_FN uint32_t pa_randint_mask(uint32_t i) {
    i |= i >> 1;
    i |= i >> 2;
    i |= i >> 4;
    i |= i >> 8;
    i |= i >> 16;
    return i;
}

// reads an interval of n reads keeps: int(min(cap, rate * n)) as Python computes it -- one double multiply, truncated toward zero
PA_RS_FN int64_t pa_reservoir_allowed(int32_t cap, double rate, int64_t n) {
    const double want = rate * (double)n;
    const double k = (double)cap < want ? (double)cap : want;
    return k > 0.0 ? (int64_t)k : 0;
}

// The draw loop over one regeneration's worth of tempered words (words[at .. count)): read i (>= k >= 1, so i >= 1 and every
// read draws) takes words until one `& mask` is <= i; a value below k puts the read into that slot.  `i` and `at` carry
// over to the next regeneration (a rejected word changes neither i nor the mask).  -> the read the loop stopped at (n: done).
PA_RS_FN int64_t pa_reservoir_draw(const uint32_t* words, int count, int* at, int64_t i, int64_t n, int64_t k, int32_t* slots) {
    int w = *at;
    while (i < n && w < count) {
        const uint32_t v = words[w++] & pa_randint_mask((uint32_t)i);
        if ((int64_t)v <= i) {
            if ((int64_t)v < k) slots[v] = (int32_t)i;
            ++i;
        }
    }
    *at = w;
    return i;
}

// the whole sample on one thread: slots[0 .. min(n, k)) (k <= 0 or n <= 0: nothing is written)
PA_RS_FN void pa_reservoir_sample_serial(uint32_t seed, int64_t n, int64_t k, int32_t* slots) {
    if (k <= 0 || n <= 0) return;
    const int64_t fill = n < k ? n : k;
    for (int64_t i = 0; i < fill; ++i) slots[i] = (int32_t)i;
    if (n <= k) return;
    uint32_t mt[PA_MT_N], words[PA_MT_N];
    pa_mt_seed(mt, seed);
    for (int64_t i = k; i < n;) {
        pa_mt_twist(mt);
        for (int p = 0; p < PA_MT_N; ++p) words[p] = pa_mt_temper(mt[p]);
        int at = 0;
        i = pa_reservoir_draw(words, PA_MT_N, &at, i, n, k, slots);
    }
}
