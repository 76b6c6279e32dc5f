// Debug aid (not product): does the chip hold a higher clock on v_mfma_f32_16x16x32_f16 than on v_mfma_f32_32x32x16_f16
// in the fused LSTM decoder's step loop (rnn_h2.hip: lstm_dec_h2_kernel)?
//   hipcc --offload-arch=gfx950 -O3 -o tools/microbench/mfma_shape tools/microbench/mfma_shape.hip && tools/microbench/mfma_shape
//   (arguments: repetitions per launch [200], passes over the table [2], rows all | dec | enc | gemm; the encoder's rows and
//   linear_1's GEMM rows are below -- the gemm rows run one pass over the k range per 50 repetitions)
// One workgroup per CU, 8 waves (two per SIMD), each with the decoder's wave tile: 64 rows x 128 columns (32 units of four
// gates), 128 accumulator registers.  A k loop of three-term split-f16 products (lo.hi, hi.lo, hi.hi) in two bodies with the
// same MFMA work:
//   S32: 24 x v_mfma_f32_32x32x16_f16 per 16-wide k step   (acc[row tile 0..1][gate] of f32x16)
//   S16: 96 x v_mfma_f32_16x16x32_f16 per 32-wide k step   (acc[row tile 0..3][gate][column tile 0..1] of f32x4)
// each in two variants:
//   reg: operands loaded once and held in registers;
//   mem: as in the decoder -- A fragments by ds_read_b128 from h2 rows in LDS (1040-byte stride), B fragments by
//        raw_buffer_load_b128 from a 3 MB block that every workgroup re-reads every 48 k16 (24 k32) steps, one memory
//        instruction per MFMA gap.  S32 keeps the decoder's 2-deep ring of whole k steps, with the 48 k steps unrolled as the
//        decoder has them ("mem-u") and as a loop of two ("mem"); S16 keeps a B ring of two stages of one gate pair each (8
//        fragments) and single-buffered A fragments that are re-read right after their last use, its k loop a loop of one
//        k32 step (unrolled over the 24 steps the compiler renames the accumulators from MFMA to MFMA, needs s_nops before
//        the loads that land in registers of MFMAs in flight, and spills).
// On random finite data and on zeros.  Reports wall TFLOP/s (hipEvents around back-to-back launches) and the in-kernel clock
// = delta s_memtime / delta s_memrealtime x 100 MHz, stamped once around the loop (median over workgroups), after at least
// 2 s of back-to-back launches of the same kernel on the same data.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

#define CHECK(x)                                                                                              \
    do {                                                                                                      \
        hipError_t e_ = (x);                                                                                  \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); }           \
    } while (0)

constexpr int ROWB = 1040, ROWD = ROWB / 4;        // h2 row of 256 units: 32 slots of (16 B hi, 16 B lo) + 16 B pad
constexpr int LDS_BYTES = 64 * ROWB;
constexpr int K16 = 48;                            // k16 steps of one decoder time step (K = 256 + 512)
constexpr unsigned W_BYTES = 4u * 8u * K16 * 2u * 1024u;   // one direction's weight fragments: 3 MB

#define GAP() __builtin_amdgcn_sched_barrier(0)

template <int SHAPE, bool MEM, bool ROLLED = false>
__global__ __launch_bounds__(512, 1) void k(int nrep, const uint32_t* __restrict__ Aimg, const uint32_t* __restrict__ Wp,
                                            float* __restrict__ out, unsigned long long* __restrict__ stamps) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int u = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < LDS_BYTES / 16; i += 512)
        reinterpret_cast<u32x4*>(lds)[i] = reinterpret_cast<const u32x4*>(Aimg)[i];
    __syncthreads();
    const unsigned woff = lane * 16u;
    unsigned long long t0, t1, r0, r1;
    float sum = 0.0f;

    if (SHAPE == 32) {
        // fragment (g, s, hi/lo) of wave u: byte (((g * 8 + u) * 48 + s) * 2 + hl) * 1024 + lane * 16
        const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint32_t*>(Wp + (size_t)u * K16 * 512), 0, (int)(W_BYTES - (unsigned)u * K16 * 2048u), 0x00020000);
        const uint32_t* arow = lds + (lane & 31) * ROWD + (lane >> 5) * 8;
        struct Frag { h8 b[4][2], a[2][2]; };
        Frag ring[2];
        auto load_b = [&](int s, Frag& fr, int g, int hl) {
            fr.b[g][hl] = __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(
                                                     wrs, woff, (unsigned)((g * 8 * K16 + s) * 2 + hl) * 1024u, 0));
        };
        auto load_a = [&](int s, Frag& fr, int m, int hl) {
            fr.a[m][hl] = *reinterpret_cast<const h8*>(arow + m * 32 * ROWD + (s & 15) * 16 + hl * 4);
        };
        f32x16 acc[2][4] = {};
#pragma unroll
        for (int i = 0; i < 8; ++i) load_b(0, ring[0], i >> 1, i & 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) load_a(0, ring[0], i >> 1, i & 1);
        GAP();
        t0 = __builtin_amdgcn_s_memtime();
        r0 = __builtin_amdgcn_s_memrealtime();
        GAP();
        auto kstep = [&](int s, int sn, int p) {
#pragma unroll
            for (int i = 0; i < 24; ++i) {
                const int term = i >> 3, g = (i & 7) >> 1, m = i & 1;
                acc[m][g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ring[p].a[m][term == 0 ? 1 : 0],
                                                                   ring[p].b[g][term == 1 ? 1 : 0], acc[m][g], 0, 0, 0);
                if (i < 16 && (i & 1)) load_b(sn, ring[p ^ 1], (i >> 1) >> 1, (i >> 1) & 1);
                if (i >= 16 && i < 20) load_a(sn, ring[p ^ 1], (i - 16) >> 1, (i - 16) & 1);
                GAP();
            }
        };
        if (MEM && ROLLED) {
            // the same stream with the k loop left as a loop of two k steps (the ring's two slots)
            for (int it = 0; it < nrep; ++it) {
#pragma unroll 1
                for (int s = 0; s < K16; s += 2) {
                    kstep(s, s + 1, 0);
                    kstep(s + 1, s + 2 < K16 ? s + 2 : 0, 1);
                }
            }
        } else if (MEM) {
            // the decoder's form: all 48 k steps of a time step unrolled
            for (int it = 0; it < nrep; ++it) {
#pragma unroll
                for (int s = 0; s < K16; ++s) kstep(s, s + 1 < K16 ? s + 1 : 0, s & 1);
            }
        } else {
            for (int it = 0; it < nrep * (K16 / 2); ++it) {
#pragma unroll
                for (int i = 0; i < 48; ++i) {
                    const int term = (i % 24) >> 3, g = (i & 7) >> 1, m = i & 1;
                    acc[m][g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ring[0].a[m][term == 0 ? 1 : 0],
                                                                       ring[0].b[g][term == 1 ? 1 : 0], acc[m][g], 0, 0, 0);
                    GAP();
                }
            }
        }
        GAP();
        t1 = __builtin_amdgcn_s_memtime();
        r1 = __builtin_amdgcn_s_memrealtime();
        GAP();
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int r = 0; r < 16; ++r) sum += acc[m][g][r];
    } else {
        // fragment (g, column tile c, k32 step s, hi/lo) of wave u: byte ((((g * 16 + 2u + c) * 24 + s) * 2 + hl) * 1024 + lane * 16
        constexpr int K32 = K16 / 2;
        const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint32_t*>(Wp + (size_t)u * 2 * K32 * 512), 0, (int)(W_BYTES - (unsigned)u * 2u * K32 * 2048u), 0x00020000);
        // lane l: row l & 15 of a row tile, 16-byte hi (then lo) slot at s * 128 + (l >> 4) * 32 of the row
        const uint32_t* arow = lds + (lane & 15) * ROWD + (lane >> 4) * 8;
        h8 a[4][2];             // [row tile][hi, lo]
        h8 b[2][2][2][2];       // [stage = gate pair][gate of the pair][column tile][hi, lo]
        auto load_b = [&](int s, int gp, int idx) {
            const int c = idx >> 2, hl = (idx >> 1) & 1, g2 = idx & 1;     // in the order the MFMAs first need them
            b[gp][g2][c][hl] = __builtin_bit_cast(
                h8, __builtin_amdgcn_raw_buffer_load_b128(
                        wrs, woff, (unsigned)((((2 * gp + g2) * 16 + c) * K32 + s) * 2 + hl) * 1024u, 0));
        };
        auto load_a = [&](int s, int m, int hl) {
            a[m][hl] = *reinterpret_cast<const h8*>(arow + m * 16 * ROWD + (s & 7) * 32 + hl * 4);
        };
        f32x4 acc[4][4][2] = {};
#pragma unroll
        for (int i = 0; i < 8; ++i) load_b(0, 0, i);
        if (!MEM) {
#pragma unroll
            for (int i = 0; i < 8; ++i) load_b(0, 1, i);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) load_a(0, i >> 1, i & 1);
        GAP();
        t0 = __builtin_amdgcn_s_memtime();
        r0 = __builtin_amdgcn_s_memrealtime();
        GAP();
        if (MEM) {
            for (int it = 0; it < nrep; ++it) {
#pragma unroll 1
                for (int s = 0; s < K32; ++s) {
#pragma unroll
                    for (int gp = 0; gp < 2; ++gp) {
                        const int sn = s + 1 < K32 ? s + 1 : 0;
#pragma unroll
                        for (int i = 0; i < 48; ++i) {
                            const int m = i / 12, c = (i % 12) / 6, term = (i % 6) >> 1, g2 = i & 1;
                            acc[m][2 * gp + g2][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                                a[m][term == 0 ? 1 : 0], b[gp][g2][c][term == 1 ? 1 : 0], acc[m][2 * gp + g2][c], 0, 0, 0);
                            // next stage's 8 B fragments (the other gate pair of this k step, or the first of the next) in
                            // the first half of the phase: the last of them has 26 MFMAs to arrive
                            if (i < 24 && i % 3 == 1) load_b(gp == 0 ? s : sn, gp ^ 1, i / 3);
                            // second gate pair: a row tile's A fragments of the next k step, right after their last use
                            if (gp == 1 && i % 12 == 9) load_a(sn, m, 1);
                            if (gp == 1 && i % 12 == 11) load_a(sn, m, 0);
                            GAP();
                        }
                    }
                }
            }
        } else {
            for (int it = 0; it < nrep * K32; ++it) {
#pragma unroll
                for (int gp = 0; gp < 2; ++gp)
#pragma unroll
                    for (int i = 0; i < 48; ++i) {
                        const int m = i / 12, c = (i % 12) / 6, term = (i % 6) >> 1, g2 = i & 1;
                        acc[m][2 * gp + g2][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                            a[m][term == 0 ? 1 : 0], b[gp][g2][c][term == 1 ? 1 : 0], acc[m][2 * gp + g2][c], 0, 0, 0);
                        GAP();
                    }
            }
        }
        GAP();
        t1 = __builtin_amdgcn_s_memtime();
        r1 = __builtin_amdgcn_s_memrealtime();
        GAP();
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int c = 0; c < 2; ++c) sum += acc[m][g][c][0] + acc[m][g][c][1] + acc[m][g][c][2] + acc[m][g][c][3];
    }
    out[blockIdx.x * 512 + tid] = sum;
    if (tid == 0) {
        stamps[blockIdx.x * 2] = t1 - t0;
        stamps[blockIdx.x * 2 + 1] = r1 - r0;
    }
}

// ---- the fused int8 ENCODER's traffic (lstm_enc_h2_kernel<2, true>): K = 256 + 32, 18 k16 = 9 k32 steps,
// one direction's fragments 1.125 MB re-read every time step, h2 rows of 1168 B ([h | x] + 16 pad).  The x steps (the last
// two k16 steps / the last k32 step) are two-term: x is int8, exact in its hi half, so lo(x).hi(w) is not issued.
//   S32: the form the encoder has today -- the 18 k16 steps of a time step unrolled, a 2-deep ring of whole k steps;
//   S16: the body it would get -- a loop over eight one-k-step bodies for h and one two-term body for x, B ring of two gate-pair
//        stages, single-buffered A re-read after its last use; the A fragments of k step 0 are read at the head of the time
//        step (in the kernel they are the h the gate phase has just written).
constexpr int EROWB = 1168, EROWD = EROWB / 4;
constexpr int ELDS_BYTES = 64 * EROWB;
constexpr int EK16 = 18, EKH16 = 16;
constexpr unsigned EW_BYTES = 4u * 8u * EK16 * 2u * 1024u;   // 1.125 MB
constexpr int EMFMA = EKH16 * 24 + (EK16 - EKH16) * 16;      // 32x32x16-equivalent MFMAs per wave and time step: 416

template <int SHAPE>
__global__ __launch_bounds__(512, 1) void ke(int nrep, const uint32_t* __restrict__ Aimg, const uint32_t* __restrict__ Wp,
                                             float* __restrict__ out, unsigned long long* __restrict__ stamps) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int u = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < ELDS_BYTES / 16; i += 512)
        reinterpret_cast<u32x4*>(lds)[i] = reinterpret_cast<const u32x4*>(Aimg)[i];
    __syncthreads();
    const unsigned woff = lane * 16u;
    unsigned long long t0, t1, r0, r1;
    float sum = 0.0f;

    if (SHAPE == 32) {
        const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint32_t*>(Wp + (size_t)u * EK16 * 512), 0, (int)(EW_BYTES - (unsigned)u * EK16 * 2048u), 0x00020000);
        const uint32_t* arow = lds + (lane & 31) * EROWD + (lane >> 5) * 8;
        struct Frag { h8 b[4][2], a[2][2]; };
        Frag ring[2];
        auto load_b = [&](int s, Frag& fr, int g, int hl) {
            fr.b[g][hl] = __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(
                                                     wrs, woff, (unsigned)((g * 8 * EK16 + s) * 2 + hl) * 1024u, 0));
        };
        auto load_a = [&](int s, Frag& fr, int m, int hl) {
            fr.a[m][hl] = *reinterpret_cast<const h8*>(arow + m * 32 * EROWD + s * 16 + hl * 4);
        };
        f32x16 acc[2][4] = {};
#pragma unroll
        for (int i = 0; i < 8; ++i) load_b(0, ring[0], i >> 1, i & 1);
        GAP();
        t0 = __builtin_amdgcn_s_memtime();
        r0 = __builtin_amdgcn_s_memrealtime();
        GAP();
        for (int it = 0; it < nrep; ++it) {
#pragma unroll
            for (int i = 0; i < 4; ++i) load_a(0, ring[0], i >> 1, i & 1);
            GAP();
#pragma unroll
            for (int s = 0; s < EK16; ++s) {
                const int p = s & 1, sn = s + 1 < EK16 ? s + 1 : 0;
                const bool two = s >= EKH16;                     // x step: hi.lo and hi.hi only
                const int n = two ? 16 : 24;
#pragma unroll
                for (int i = 0; i < n; ++i) {
                    const int term = (i >> 3) + (two ? 1 : 0), g = (i & 7) >> 1, m = i & 1;
                    acc[m][g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ring[p].a[m][term == 0 ? 1 : 0],
                                                                       ring[p].b[g][term == 1 ? 1 : 0], acc[m][g], 0, 0, 0);
                    if (!two) {
                        if (i < 16 && (i & 1)) load_b(sn, ring[p ^ 1], (i >> 1) >> 1, (i >> 1) & 1);
                        if (i >= 16 && i < 20) load_a(sn, ring[p ^ 1], (i - 16) >> 1, (i - 16) & 1);
                    } else {
                        if (i < 8) load_b(sn, ring[p ^ 1], i >> 1, i & 1);
                        if (sn != 0 && i >= 8 && i < 12) load_a(sn, ring[p ^ 1], (i - 8) >> 1, (i - 8) & 1);
                    }
                    GAP();
                }
            }
        }
        GAP();
        t1 = __builtin_amdgcn_s_memtime();
        r1 = __builtin_amdgcn_s_memrealtime();
        GAP();
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int r = 0; r < 16; ++r) sum += acc[m][g][r];
    } else {
        constexpr int K32 = EK16 / 2, KH32 = EKH16 / 2;
        const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint32_t*>(Wp + (size_t)u * 2 * K32 * 512), 0, (int)(EW_BYTES - (unsigned)u * 2u * K32 * 2048u), 0x00020000);
        const uint32_t* arow = lds + (lane & 15) * EROWD + (lane >> 4) * 8;
        h8 a[4][2];             // [row tile][hi, lo]
        h8 b[2][2][2][2];       // [stage = gate pair][gate of the pair][column tile][hi, lo]
        auto load_b = [&](int s, int gp, int idx) {
            const int c = idx >> 2, hl = (idx >> 1) & 1, g2 = idx & 1;
            b[gp][g2][c][hl] = __builtin_bit_cast(
                h8, __builtin_amdgcn_raw_buffer_load_b128(
                        wrs, woff, (unsigned)((((2 * gp + g2) * 16 + c) * K32 + s) * 2 + hl) * 1024u, 0));
        };
        auto load_a = [&](int s, int m, int hl) {
            a[m][hl] = *reinterpret_cast<const h8*>(arow + m * 16 * EROWD + s * 32 + hl * 4);
        };
        f32x4 acc[4][4][2] = {};
        int once = 1;
        asm volatile("" : "+s"(once));
#pragma unroll
        for (int i = 0; i < 8; ++i) load_b(0, 0, i);
        GAP();
        t0 = __builtin_amdgcn_s_memtime();
        r0 = __builtin_amdgcn_s_memrealtime();
        GAP();
        for (int it = 0; it < nrep; ++it) {
#pragma unroll
            for (int i = 0; i < 8; ++i) load_a(0, i >> 1, i & 1);
            GAP();
#pragma unroll 1
            for (int s = 0; s < KH32; ++s) {
#pragma unroll
                for (int gp = 0; gp < 2; ++gp)
#pragma unroll
                    for (int i = 0; i < 48; ++i) {
                        const int m = i / 12, c = (i % 12) / 6, term = (i % 6) >> 1, g2 = i & 1;
                        acc[m][2 * gp + g2][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                            a[m][term == 0 ? 1 : 0], b[gp][g2][c][term == 1 ? 1 : 0], acc[m][2 * gp + g2][c], 0, 0, 0);
                        if (i < 24 && i % 3 == 1) load_b(gp == 0 ? s : s + 1, gp ^ 1, i / 3);
                        // the x step wants no lo half of A
                        if (gp == 1 && i % 12 == 9 && s + 1 < KH32) load_a(s + 1, m, 1);
                        if (gp == 1 && i % 12 == 11) load_a(s + 1, m, 0);
                        GAP();
                    }
            }
#pragma unroll 1
            for (int r = 0; r < once; ++r) {
#pragma unroll
                for (int gp = 0; gp < 2; ++gp)
#pragma unroll
                    for (int i = 0; i < 32; ++i) {
                        const int m = i / 8, c = (i % 8) / 4, term = 1 + ((i % 4) >> 1), g2 = i & 1;
                        acc[m][2 * gp + g2][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                            a[m][0], b[gp][g2][c][term == 1 ? 1 : 0], acc[m][2 * gp + g2][c], 0, 0, 0);
                        if (i < 16 && (i & 1)) load_b(gp == 0 ? KH32 : 0, gp ^ 1, i >> 1);
                        GAP();
                    }
            }
        }
        GAP();
        t1 = __builtin_amdgcn_s_memtime();
        r1 = __builtin_amdgcn_s_memrealtime();
        GAP();
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int c = 0; c < 2; ++c) sum += acc[m][g][c][0] + acc[m][g][c][1] + acc[m][g][c][2] + acc[m][g][c][3];
    }
    out[blockIdx.x * 512 + tid] = sum;
    if (tid == 0) {
        stamps[blockIdx.x * 2] = t1 - t0;
        stamps[blockIdx.x * 2 + 1] = r1 - r0;
    }
}

// ---- linear_1's split-K GEMM (gemm_h2.hip: gemm_h2_kernel<0>, M = 16 384, N = 512, K = 16 896, two k slices): the real
// grid (64 x 2 tiles of 256 x 256, two slices = 256 workgroups), the real operands (row-major h2, 1.1 GB of A), the real
// staging: per k-tile of 32 and workgroup 16 buffer_load_b128 per 256 threads into staging registers, 16 ds_write_b128 into
// two stages of 512 rows x 144 B, one barrier, every fragment by ds_read_b128.  Three bodies:
//   a: the kernel as it is -- 4 waves, 128 x 128 wave tile, 96 x 32x32x16 per k-tile, two fragment sets, the k-tile body
//      scheduled by sched_group_barrier;
//   b: 4 waves, 128 x 128 wave tile as 8 x 8 tiles of 16 x 16 (256 accumulator registers), 192 x 16x16x32 per k-tile, one
//      fragment set re-read right after its last use (row tile m after row m, the column tiles through the last row), the
//      barrier after the first row, a loop over one-k-tile bodies;
//   c: 8 waves (two per SIMD), 128 x 64 wave tile (128 accumulator registers), 96 x 16x16x32 per wave and k-tile, the same
//      staging over 512 threads (8 loads each), A fragments as a ring of two row tiles (the whole set does not fit 256
//      registers beside the staging), B fragments re-read through the last row; 1.5 x the fragment reads of a and b.
// The accumulators are summed, not stored: the epilogue is not part of the question.
constexpr int GT = 256, GK = 32, GROW = 36, GSTAGE = 2 * GT * GROW;     // tile, k-tile, LDS row (dwords), stage (dwords)
constexpr int G_M = 16384, G_N = 512, G_K = 16896, G_SPLITS = 2;
constexpr int G_TILES_N = G_N / GT, G_NWG = (G_M / GT) * G_TILES_N, G_NK = G_K / GK / G_SPLITS;

__device__ __forceinline__ void lds_barrier() {      // s_waitcnt lgkmcnt(0) + s_barrier: global loads stay in flight
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <int BODY>
__global__ __launch_bounds__(BODY == 2 ? 512 : 256) void kg(int nrep, const uint32_t* __restrict__ A, const uint32_t* __restrict__ W,
                                                            float* __restrict__ out, unsigned long long* __restrict__ stamps) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[2 * GSTAGE];
    constexpr int NT = BODY == 2 ? 512 : 256, NP = BODY == 2 ? 4 : 8;     // threads, staged rows of A (and of W) per thread
    // gemm_h2_kernel's tile order: XCD-contiguous runs, groups of 4 row panels, row panel fastest
    int tile;
    {
        const int bid = blockIdx.x, q = G_NWG >> 3;
        tile = (bid & 7) * q + (bid >> 3);
    }
    const int group = tile / (4 * G_TILES_N), within = tile - group * (4 * G_TILES_N);
    const int m0 = (group * 4 + within % 4) * GT, n0 = (within / 4) * GT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = tid & 7, r0 = tid >> 3;
    const __amdgpu_buffer_rsrc_t arsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(A), 0, (int)((unsigned)G_M * G_K * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(W), 0, (int)((unsigned)G_N * G_K * 4u), 0x00020000);
    uint32_t aoff[NP], woff[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        aoff[i] = (uint32_t)(m0 + r0 + (NT / 8) * i) * (G_K * 4u) + kq * 16;
        woff[i] = (uint32_t)(n0 + r0 + (NT / 8) * i) * (G_K * 4u) + kq * 16;
    }
    u32x4 ra[NP], rb[NP];
    auto gload1 = [&](int kt, int i) {     // piece i < NP: A, else W
        if (i < NP) ra[i] = __builtin_amdgcn_raw_buffer_load_b128(arsrc, aoff[i], kt * (GK * 4), 0);
        else rb[i - NP] = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, woff[i - NP], kt * (GK * 4), 0);
    };
    auto lstore1 = [&](int buf, int i) {
        uint32_t* base = lds + buf * GSTAGE + r0 * GROW + kq * 4;
        if (i < NP) *reinterpret_cast<u32x4*>(base + ((NT / 8) * i) * GROW) = ra[i];
        else *reinterpret_cast<u32x4*>(base + (GT + (NT / 8) * (i - NP)) * GROW) = rb[i - NP];
    };
    const int kbeg = G_NK * (int)blockIdx.y, nk = G_NK;
    unsigned long long t0, t1, c0, c1;
    float sum = 0.0f;
    GAP();
    t0 = __builtin_amdgcn_s_memtime();
    c0 = __builtin_amdgcn_s_memrealtime();
    GAP();

    if constexpr (BODY == 0) {
        const int wm = wid >> 1, wn = wid & 1, li = lane & 31, hf = lane >> 5;
        f32x16 acc[4][4] = {};
        struct Frag { h8 a[4][2], b[4][2]; };
        auto read_step = [&](int buf, int step, Frag& f) {
            const uint32_t* Ab = lds + buf * GSTAGE + (wm * 128 + li) * GROW + (2 * step + hf) * 8;
            const uint32_t* Bb = lds + buf * GSTAGE + (GT + wn * 128 + li) * GROW + (2 * step + hf) * 8;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                f.a[m][0] = *reinterpret_cast<const h8*>(Ab + m * 32 * GROW);
                f.a[m][1] = *reinterpret_cast<const h8*>(Ab + m * 32 * GROW + 4);
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                f.b[n][0] = *reinterpret_cast<const h8*>(Bb + n * 32 * GROW);
                f.b[n][1] = *reinterpret_cast<const h8*>(Bb + n * 32 * GROW + 4);
            }
        };
        auto mma_step = [&](const Frag& f) {
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int n = 0; n < 4; ++n)
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[m][t == 0 ? 1 : 0], f.b[n][t == 1 ? 1 : 0],
                                                                           acc[m][n], 0, 0, 0);
        };
        Frag f0, f1;
        for (int rep = 0; rep < nrep; ++rep) {
#pragma unroll
            for (int i = 0; i < 16; ++i) gload1(kbeg, i);
#pragma unroll
            for (int i = 0; i < 16; ++i) lstore1(0, i);
#pragma unroll
            for (int i = 0; i < 16; ++i) gload1(kbeg + (nk > 1 ? 1 : 0), i);
            __syncthreads();
            read_step(0, 0, f0);
            for (int kt = 0; kt < nk; ++kt) {
                const int buf = kt & 1;
                const int nxt2 = kbeg + (kt + 2 < nk ? kt + 2 : nk - 1);
                read_step(buf, 1, f1);
#pragma unroll
                for (int i = 0; i < 8; ++i) { lstore1(buf ^ 1, i); lstore1(buf ^ 1, 8 + i); }
#pragma unroll
                for (int i = 0; i < 8; ++i) gload1(nxt2, i);
                mma_step(f0);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
                __builtin_amdgcn_sched_barrier(0);
                __syncthreads();
                read_step(buf ^ 1, 0, f0);
#pragma unroll
                for (int i = 8; i < 16; ++i) gload1(nxt2, i);
                mma_step(f1);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 24, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();     // the next repetition's prologue writes stage 0
        }
        GAP();
        t1 = __builtin_amdgcn_s_memtime();
        c1 = __builtin_amdgcn_s_memrealtime();
        GAP();
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) sum += acc[m][n][r];
    } else if constexpr (BODY == 1) {
        const int wm = wid >> 1, wn = wid & 1, l15 = lane & 15, qd = lane >> 4;
        // lane l: row l & 15 of a 16-row tile, k 8 (l >> 4) .. + 7 of the k-tile: 16 B hi at byte 32 (l >> 4), lo 16 B on
        const uint32_t* afr = lds + (wm * 128 + l15) * GROW + qd * 8;
        const uint32_t* bfr = lds + (GT + wn * 128 + l15) * GROW + qd * 8;
        h8 a[8][2], b[8][2];       // [tile][hi, lo], one set
        f32x4 acc[8][8] = {};
        auto rd_a = [&](int buf, int m, int hl) { a[m][hl] = *reinterpret_cast<const h8*>(afr + buf * GSTAGE + m * 16 * GROW + hl * 4); };
        auto rd_b = [&](int buf, int n, int hl) { b[n][hl] = *reinterpret_cast<const h8*>(bfr + buf * GSTAGE + n * 16 * GROW + hl * 4); };
        for (int rep = 0; rep < nrep; ++rep) {
            // stage 0 <- tile 0, stage 1 <- tile 1, staging registers <- tile 2 (indices clamped to the slice)
#pragma unroll
            for (int i = 0; i < 16; ++i) gload1(kbeg, i);
#pragma unroll
            for (int i = 0; i < 16; ++i) lstore1(0, i);
#pragma unroll
            for (int i = 0; i < 16; ++i) gload1(kbeg + (nk > 1 ? 1 : 0), i);
#pragma unroll
            for (int i = 0; i < 16; ++i) lstore1(1, i);
#pragma unroll
            for (int i = 0; i < 16; ++i) gload1(kbeg + (nk > 2 ? 2 : nk - 1), i);
            __syncthreads();
#pragma unroll
            for (int n = 0; n < 8; ++n) { rd_b(0, n, 0); rd_b(0, n, 1); }
#pragma unroll
            for (int m = 0; m < 7; ++m) { rd_a(0, m, 0); rd_a(0, m, 1); }
            GAP();
            // Tile t: the registers hold its fragments but row tile 7's, which row 0 reads from stage t & 1.  The barrier
            // after row 0 says: every wave has read all it wants of stage t & 1 (tile t+2 may be written there) and tile
            // t+1 is whole in the other stage (written during tile t-1).  Rows 1 .. 6: tile t+2 from the staging registers
            // to LDS, each piece's request for tile t+3 behind it.  Row m: row tile m-1 of tile t+1.  Row 7: the column
            // tiles of tile t+1, each pair after its last MFMA.
#pragma unroll 1
            for (int t = 0; t < nk; ++t) {
                const int cur = t & 1, nxt = cur ^ 1;
                const int kt3 = kbeg + (t + 3 < nk ? t + 3 : nk - 1);
#pragma unroll
                for (int m = 0; m < 8; ++m)
#pragma unroll
                for (int r = 0; r < 24; ++r) {
                    const int n = 2 * (r / 6) + (r & 1), term = (r % 6) >> 1;
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[m][term == 0 ? 1 : 0], b[n][term == 1 ? 1 : 0],
                                                                       acc[m][n], 0, 0, 0);
                    if (m == 0) {
                        if (r == 0) rd_a(cur, 7, 1);
                        if (r == 1) rd_a(cur, 7, 0);
                        if (r == 23) { GAP(); lds_barrier(); }
                    } else {
                        if (r == 2) rd_a(nxt, m - 1, 1);
                        if (r == 8) rd_a(nxt, m - 1, 0);
                        const int g = (m - 1) * 24 + r;      // rows 1 .. 6: a piece every 9 gaps (the slow LDS write port)
                        if (m <= 6 && g % 9 == 0) lstore1(cur, g / 9);
                        if (m <= 6 && g % 9 == 1) gload1(kt3, g / 9);
                        if (m == 7 && r % 6 == 3) rd_b(nxt, n - 1, 1);
                        if (m == 7 && r % 6 == 4) rd_b(nxt, n + 1, 1);
                        if (m == 7 && r % 6 == 5) { rd_b(nxt, n - 1, 0); rd_b(nxt, n, 0); }
                    }
                    GAP();
                }
            }
            __syncthreads();
        }
        GAP();
        t1 = __builtin_amdgcn_s_memtime();
        c1 = __builtin_amdgcn_s_memrealtime();
        GAP();
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int n = 0; n < 8; ++n) sum += acc[m][n][0] + acc[m][n][1] + acc[m][n][2] + acc[m][n][3];
    } else {
        const int wm = wid >> 2, wn = wid & 3, l15 = lane & 15, qd = lane >> 4;
        const uint32_t* afr = lds + (wm * 128 + l15) * GROW + qd * 8;
        const uint32_t* bfr = lds + (GT + wn * 64 + l15) * GROW + qd * 8;
        h8 a[2][2], b[4][2];       // A: ring of two row tiles; B: one set
        f32x4 acc[8][4] = {};
        auto rd_a = [&](int buf, int m, int hl) { a[m & 1][hl] = *reinterpret_cast<const h8*>(afr + buf * GSTAGE + m * 16 * GROW + hl * 4); };
        auto rd_b = [&](int buf, int n, int hl) { b[n][hl] = *reinterpret_cast<const h8*>(bfr + buf * GSTAGE + n * 16 * GROW + hl * 4); };
        for (int rep = 0; rep < nrep; ++rep) {
#pragma unroll
            for (int i = 0; i < 8; ++i) gload1(kbeg, i);
#pragma unroll
            for (int i = 0; i < 8; ++i) lstore1(0, i);
#pragma unroll
            for (int i = 0; i < 8; ++i) gload1(kbeg + (nk > 1 ? 1 : 0), i);
            __syncthreads();
#pragma unroll
            for (int n = 0; n < 4; ++n) { rd_b(0, n, 0); rd_b(0, n, 1); }
            rd_a(0, 0, 0); rd_a(0, 0, 1);
            GAP();
            // Tile t: row m reads row tile m+1 of stage t & 1 into the other ring slot.  Rows 0 .. 5: tile t+1 from the
            // staging registers to the other stage, each piece's request for tile t+2 behind it.  The barrier before row 7
            // says: stage t & 1 is read out and tile t+1 is whole.  Row 7: row tile 0 and the column tiles of tile t+1.
#pragma unroll 1
            for (int t = 0; t < nk; ++t) {
                const int cur = t & 1, nxt = cur ^ 1;
                const int kt2 = kbeg + (t + 2 < nk ? t + 2 : nk - 1);
#pragma unroll
                for (int m = 0; m < 8; ++m)
#pragma unroll
                for (int r = 0; r < 12; ++r) {
                    const int n = 2 * (r / 6) + (r & 1), term = (r % 6) >> 1;
                    if (m == 7 && r == 0) { lds_barrier(); GAP(); }
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[m & 1][term == 0 ? 1 : 0], b[n][term == 1 ? 1 : 0],
                                                                       acc[m][n], 0, 0, 0);
                    if (r == 0) rd_a(m < 7 ? cur : nxt, (m + 1) & 7, 1);
                    if (r == 1) rd_a(m < 7 ? cur : nxt, (m + 1) & 7, 0);
                    const int g = m * 12 + r;               // rows 0 .. 5: a piece every 9 gaps
                    if (m <= 5 && g % 9 == 2) lstore1(nxt, g / 9);
                    if (m <= 5 && g % 9 == 3) gload1(kt2, g / 9);
                    if (m == 7 && r % 6 == 3) rd_b(nxt, n - 1, 1);
                    if (m == 7 && r % 6 == 4) rd_b(nxt, n + 1, 1);
                    if (m == 7 && r % 6 == 5) { rd_b(nxt, n - 1, 0); rd_b(nxt, n, 0); }
                    GAP();
                }
            }
            __syncthreads();
        }
        GAP();
        t1 = __builtin_amdgcn_s_memtime();
        c1 = __builtin_amdgcn_s_memrealtime();
        GAP();
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) sum += acc[m][n][0] + acc[m][n][1] + acc[m][n][2] + acc[m][n][3];
    }
    out[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NT + tid] = sum;
    if (tid == 0) {
        stamps[(blockIdx.y * gridDim.x + blockIdx.x) * 2] = t1 - t0;
        stamps[(blockIdx.y * gridDim.x + blockIdx.x) * 2 + 1] = c1 - c0;
    }
}

static uint16_t f16_bits(_Float16 h) { uint16_t b; memcpy(&b, &h, 2); return b; }

// nwords 32-byte h2 slots (8 values: 16 B hi, 16 B lo) of uniform values in [-scale, scale), or zeros
static void fill_h2(uint16_t* dst, size_t nslots, bool random, float scale, unsigned& seed) {
    for (size_t s = 0; s < nslots; ++s)
        for (int e = 0; e < 8; ++e) {
            seed = seed * 1664525u + 1013904223u;
            const float v = random ? scale * ((float)(seed >> 8) * (2.0f / 16777216.0f) - 1.0f) : 0.0f;
            const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi);
            dst[s * 16 + e] = f16_bits(hi);
            dst[s * 16 + 8 + e] = f16_bits(lo);
        }
}

struct Bufs { uint32_t *aimg, *w; float* out; unsigned long long* stamps; int ncu; };

template <int SHAPE, bool MEM, bool ROLLED = false>
void run(const Bufs& d, const char* data, int nrep) {
    auto fn = k<SHAPE, MEM, ROLLED>;
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    auto launch = [&]() { hipLaunchKernelGGL(fn, dim3(d.ncu), dim3(512), LDS_BYTES, 0, nrep, d.aimg, d.w, d.out, d.stamps); };
    // at least 2 s of back-to-back launches before anything is read
    const auto w0 = std::chrono::steady_clock::now();
    int warm = 0;
    do {
        for (int i = 0; i < 8; ++i) launch();
        CHECK(hipDeviceSynchronize());
        warm += 8;
    } while (std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() < 2.0);
    constexpr int L = 40;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    CHECK(hipEventRecord(e0, 0));
    for (int i = 0; i < L; ++i) launch();
    CHECK(hipEventRecord(e1, 0));
    CHECK(hipEventSynchronize(e1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> st(2 * d.ncu);
    CHECK(hipMemcpy(st.data(), d.stamps, st.size() * 8, hipMemcpyDeviceToHost));
    std::vector<double> ghz(d.ncu);
    for (int i = 0; i < d.ncu; ++i) ghz[i] = 0.1 * (double)st[2 * i] / (double)st[2 * i + 1];
    std::sort(ghz.begin(), ghz.end());
    // per wave and k16 step: 24 MFMAs of 2 * 32 * 32 * 16 FLOP (= 96 of 2 * 16 * 16 * 32 per two of them)
    const double flop = (double)L * d.ncu * 8.0 * nrep * K16 * 24.0 * 32768.0;
    // two waves share a SIMD: cycles of the launch (wall x in-kernel clock, so launch overhead and the LDS fill included) per
    // 32x32x16-equivalent MFMA of the pair; the pipe's own figure is 32
    const double cpm = (double)ms / L * 1e6 * ghz[d.ncu / 2] / ((double)nrep * K16 * 24.0 * 2.0);
    printf("%-9s %-5s %-6s  %8.3f ms/launch  %8.1f TFLOP/s  clock %.3f GHz  %6.2f SIMD cycles per 32x32x16-equivalent MFMA  (%d warm launches)\n",
           SHAPE == 32 ? "32x32x16" : "16x16x32", !MEM ? "reg" : SHAPE == 32 && !ROLLED ? "mem-u" : "mem", data, ms / L, flop / (ms * 1e-3) * 1e-12, ghz[d.ncu / 2], cpm, warm);
    fflush(stdout);
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
}

template <int SHAPE>
void run_enc(const Bufs& d, const char* data, int nrep) {
    auto fn = ke<SHAPE>;
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, ELDS_BYTES));
    auto launch = [&]() { hipLaunchKernelGGL(fn, dim3(d.ncu), dim3(512), ELDS_BYTES, 0, nrep, d.aimg, d.w, d.out, d.stamps); };
    const auto w0 = std::chrono::steady_clock::now();
    int warm = 0;
    do {
        for (int i = 0; i < 8; ++i) launch();
        CHECK(hipDeviceSynchronize());
        warm += 8;
    } while (std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() < 2.0);
    constexpr int L = 40;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    CHECK(hipEventRecord(e0, 0));
    for (int i = 0; i < L; ++i) launch();
    CHECK(hipEventRecord(e1, 0));
    CHECK(hipEventSynchronize(e1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> st(2 * d.ncu);
    CHECK(hipMemcpy(st.data(), d.stamps, st.size() * 8, hipMemcpyDeviceToHost));
    std::vector<double> ghz(d.ncu);
    for (int i = 0; i < d.ncu; ++i) ghz[i] = 0.1 * (double)st[2 * i] / (double)st[2 * i + 1];
    std::sort(ghz.begin(), ghz.end());
    const double flop = (double)L * d.ncu * 8.0 * nrep * EMFMA * 32768.0;
    const double cpm = (double)ms / L * 1e6 * ghz[d.ncu / 2] / ((double)nrep * EMFMA * 2.0);
    printf("%-9s %-5s %-6s  %8.3f ms/launch  %8.1f TFLOP/s  clock %.3f GHz  %6.2f SIMD cycles per 32x32x16-equivalent MFMA  (%d warm launches)\n",
           SHAPE == 32 ? "32x32x16" : "16x16x32", "enc", data, ms / L, flop / (ms * 1e-3) * 1e-12, ghz[d.ncu / 2], cpm, warm);
    fflush(stdout);
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
}

// the encoder rows: its own LDS image ([h | x] rows of 1168 B, x = int8 values in the hi half) and weight block (1.125 MB)
static void enc_rows(const Bufs& d, int nrep, int passes) {
    printf("encoder traffic: %d x %d k16 steps per launch\n", nrep, EK16);
    std::vector<uint16_t> ha(ELDS_BYTES / 2, 0), hw(EW_BYTES / 2);
    for (int pass = 0; pass < passes; ++pass)
        for (int rnd = 1; rnd >= 0; --rnd) {
            unsigned seed = 12345u;
            for (int r = 0; r < 64; ++r) {
                uint16_t* row = ha.data() + (size_t)r * (EROWB / 2);
                fill_h2(row, 32, rnd, 1.0f, seed);                        // h in (-1, 1)
                for (int sl = 32; sl < 36; ++sl)
                    for (int e = 0; e < 8; ++e) {                         // x: an int8 value, lo half zero
                        seed = seed * 1664525u + 1013904223u;
                        row[sl * 16 + e] = f16_bits((_Float16)(rnd ? (float)((int)(seed >> 24) - 128) : 0.0f));
                        row[sl * 16 + 8 + e] = 0;
                    }
            }
            for (size_t f = 0; f < EW_BYTES / 2048; ++f) {
                std::vector<uint16_t> tmp(1024);
                fill_h2(tmp.data(), 64, rnd, 0.5f, seed);
                for (int s = 0; s < 64; ++s) {
                    memcpy(&hw[f * 1024 + s * 8], &tmp[s * 16], 16);
                    memcpy(&hw[f * 1024 + 512 + s * 8], &tmp[s * 16 + 8], 16);
                }
            }
            CHECK(hipMemcpy(d.aimg, ha.data(), ELDS_BYTES, hipMemcpyHostToDevice));
            CHECK(hipMemcpy(d.w, hw.data(), EW_BYTES, hipMemcpyHostToDevice));
            const char* data = rnd ? "random" : "zeros";
            run_enc<32>(d, data, nrep);
            run_enc<16>(d, data, nrep);
        }
}

template <int BODY>
void run_gemm(const uint32_t* A, const uint32_t* W, float* out, unsigned long long* stamps, const char* data, int nrep) {
    constexpr int NT = BODY == 2 ? 512 : 256;
    auto launch = [&]() { hipLaunchKernelGGL(kg<BODY>, dim3(G_NWG, G_SPLITS), dim3(NT), 0, 0, nrep, A, W, out, stamps); };
    const auto w0 = std::chrono::steady_clock::now();
    int warm = 0;
    do {
        for (int i = 0; i < 8; ++i) launch();
        CHECK(hipDeviceSynchronize());
        warm += 8;
    } while (std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() < 2.0);
    constexpr int L = 40, NW = G_NWG * G_SPLITS;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    CHECK(hipEventRecord(e0, 0));
    for (int i = 0; i < L; ++i) launch();
    CHECK(hipEventRecord(e1, 0));
    CHECK(hipEventSynchronize(e1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> st(2 * NW);
    CHECK(hipMemcpy(st.data(), stamps, st.size() * 8, hipMemcpyDeviceToHost));
    std::vector<double> ghz(NW);
    for (int i = 0; i < NW; ++i) ghz[i] = 0.1 * (double)st[2 * i] / (double)st[2 * i + 1];
    std::sort(ghz.begin(), ghz.end());
    const double flop = (double)L * nrep * 3.0 * 2.0 * G_M * G_N * G_K;
    // one workgroup per CU: per SIMD and k-tile 96 32x32x16-equivalent MFMAs (one wave's, or two waves' 48 each)
    const double cpm = (double)ms / L * 1e6 * ghz[NW / 2] / ((double)nrep * G_NK * 96.0);
    printf("%-9s %-5s %-6s  %8.3f ms/launch  %8.1f TFLOP/s  clock %.3f GHz  %6.2f SIMD cycles per 32x32x16-equivalent MFMA  (%d warm launches)\n",
           BODY == 0 ? "32x32x16" : "16x16x32", BODY == 0 ? "gemm-a" : BODY == 1 ? "gemm-b" : "gemm-c", data, ms / L,
           flop / (ms * 1e-3) * 1e-12, ghz[NW / 2], cpm, warm);
    fflush(stdout);
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
}

// the gemm rows: linear_1's operands at full size, A as copies of one random 1024-row block
static void gemm_rows(int nrep, int passes) {
    printf("linear_1 GEMM traffic: M %d, N %d, K %d in %d slices, %d x %d k-tiles of 32 per workgroup and launch\n", G_M, G_N, G_K,
           G_SPLITS, nrep, G_NK);
    const size_t a_bytes = (size_t)G_M * G_K * 4, w_bytes = (size_t)G_N * G_K * 4, blk_rows = 1024, blk = blk_rows * G_K * 4;
    uint32_t *A, *W;
    float* out;
    unsigned long long* stamps;
    CHECK(hipMalloc(&A, a_bytes)); CHECK(hipMalloc(&W, w_bytes));
    CHECK(hipMalloc(&out, (size_t)G_NWG * G_SPLITS * 512 * 4)); CHECK(hipMalloc(&stamps, (size_t)G_NWG * G_SPLITS * 16));
    std::vector<uint16_t> ha(blk / 2), hw(w_bytes / 2);
    for (int pass = 0; pass < passes; ++pass)
        for (int rnd = 1; rnd >= 0; --rnd) {
            if (rnd) {
                unsigned seed = 12345u;
                fill_h2(ha.data(), blk / 32, true, 1.0f, seed);      // the decoder's h in (-1, 1)
                fill_h2(hw.data(), w_bytes / 32, true, 0.5f, seed);
                CHECK(hipMemcpy(W, hw.data(), w_bytes, hipMemcpyHostToDevice));
                CHECK(hipMemcpy(A, ha.data(), blk, hipMemcpyHostToDevice));
                for (size_t r = blk_rows; r < (size_t)G_M; r += blk_rows)
                    CHECK(hipMemcpy(reinterpret_cast<char*>(A) + r * G_K * 4, A, blk, hipMemcpyDeviceToDevice));
            } else {
                CHECK(hipMemset(A, 0, a_bytes));
                CHECK(hipMemset(W, 0, w_bytes));
            }
            CHECK(hipDeviceSynchronize());
            const char* data = rnd ? "random" : "zeros";
            run_gemm<0>(A, W, out, stamps, data, nrep);
            run_gemm<1>(A, W, out, stamps, data, nrep);
            run_gemm<2>(A, W, out, stamps, data, nrep);
        }
    CHECK(hipFree(A)); CHECK(hipFree(W)); CHECK(hipFree(out)); CHECK(hipFree(stamps));
}

int main(int argc, char** argv) {
    const int nrep = argc > 1 ? atoi(argv[1]) : 200, passes = argc > 2 ? atoi(argv[2]) : 2;
    const char* rows = argc > 3 ? argv[3] : "all";      // all | dec | enc | gemm
    const bool all = strcmp(rows, "all") == 0;
    const bool dec = all || strcmp(rows, "dec") == 0, enc = all || strcmp(rows, "enc") == 0;    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    Bufs d;
    d.ncu = prop.multiProcessorCount;
    CHECK(hipMalloc(&d.aimg, ELDS_BYTES)); CHECK(hipMalloc(&d.w, W_BYTES));
    CHECK(hipMalloc(&d.out, (size_t)d.ncu * 512 * 4)); CHECK(hipMalloc(&d.stamps, (size_t)d.ncu * 16));
    printf("%s, %d CUs, %d x %d k16 steps per launch\n", prop.name, d.ncu, nrep, K16);
    std::vector<uint16_t> ha(LDS_BYTES / 2, 0), hw(W_BYTES / 2);
    for (int pass = 0; dec && pass < passes; ++pass)
        for (int rnd = 1; rnd >= 0; --rnd) {
            unsigned seed = 12345u;
            for (int r = 0; r < 64; ++r) fill_h2(ha.data() + (size_t)r * (ROWB / 2), 32, rnd, 1.0f, seed);   // h in (-1, 1)
            // a weight fragment pair is 1024 B hi then 1024 B lo; which value sits where does not matter to the probe
            for (size_t f = 0; f < W_BYTES / 2048; ++f) {
                std::vector<uint16_t> tmp(1024);
                fill_h2(tmp.data(), 64, rnd, 0.5f, seed);
                for (int s = 0; s < 64; ++s) {
                    memcpy(&hw[f * 1024 + s * 8], &tmp[s * 16], 16);
                    memcpy(&hw[f * 1024 + 512 + s * 8], &tmp[s * 16 + 8], 16);
                }
            }
            CHECK(hipMemcpy(d.aimg, ha.data(), LDS_BYTES, hipMemcpyHostToDevice));
            CHECK(hipMemcpy(d.w, hw.data(), W_BYTES, hipMemcpyHostToDevice));
            const char* data = rnd ? "random" : "zeros";
            run<32, false>(d, data, nrep);
            run<16, false>(d, data, nrep);
            run<32, true>(d, data, nrep);
            run<32, true, true>(d, data, nrep);
            run<16, true>(d, data, nrep);
        }
    if (enc) enc_rows(d, nrep * K16 / EK16, passes);
    if (all || strcmp(rows, "gemm") == 0) gemm_rows(std::max(1, nrep / 50), passes);
    CHECK(hipFree(d.aimg)); CHECK(hipFree(d.w)); CHECK(hipFree(d.out)); CHECK(hipFree(d.stamps));
    return 0;
}
