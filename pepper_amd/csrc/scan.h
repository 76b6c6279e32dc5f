// Exclusive scan on the device, reduce-then-scan over separate launches (block sums, scan of the sums, add back): no workgroup
// ever waits for another one, and the result does not depend on the order the workgroups run in.  Shared by the polish stitch
// (stitch.hip) and the candidate selection (select.hip); everything lives in an unnamed namespace, so each file that includes
// this header gets its own instances of the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"

namespace {

constexpr int ST_THREADS = 256;                         // 4 waves
constexpr int ST_ITEMS = 4;                             // consecutive scan elements per thread
constexpr int ST_B = ST_THREADS * ST_ITEMS;             // scan elements per workgroup

struct LoadU32 {
    const uint32_t* p;
    PA_DEV uint64_t operator()(uint64_t i) const { return p[i]; }
};
struct LoadU64 {
    const uint64_t* p;
    PA_DEV uint64_t operator()(uint64_t i) const { return p[i]; }
};

PA_DEV uint64_t shfl_up64(uint64_t v, int d) {
    const int lo = __shfl_up((int)(uint32_t)v, d), hi = __shfl_up((int)(uint32_t)(v >> 32), d);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

// inclusive scan of one value per thread over the workgroup -> (inclusive prefix, workgroup total)
PA_DEV uint64_t block_scan(uint64_t v, uint64_t* s_wave, uint64_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t u = shfl_up64(v, d);
        if (lane >= d) v += u;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (int w = 0; w < ST_THREADS / 64; ++w) {
        if (w < wave) before += s_wave[w];
        all += s_wave[w];
    }
    *total = all;
    return v + before;
}

// sums[b] = sum of in[b * B .. min(n, (b + 1) * B))  (a workgroup past the end writes 0)
template <class L>
__global__ __launch_bounds__(ST_THREADS) void k_scan_reduce(L in, uint64_t n, uint64_t* __restrict__ sums) {
    __shared__ uint64_t s_wave[ST_THREADS / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * ST_B + (uint64_t)threadIdx.x * ST_ITEMS;
    uint64_t v = 0;
    for (int k = 0; k < ST_ITEMS; ++k)
        if (i0 + k < n) v += in(i0 + k);
    uint64_t total;
    (void)block_scan(v, s_wave, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// out[i] = offset[b] + sum of in[b * B .. i)   (offset == nullptr: one workgroup, offset 0).  in and out may be the same array:
// a thread reads its own elements before it writes them and touches no others.
template <class L, class TO>
__global__ __launch_bounds__(ST_THREADS) void k_scan_down(L in, uint64_t n, const uint64_t* __restrict__ offset, TO* out) {
    __shared__ uint64_t s_wave[ST_THREADS / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * ST_B + (uint64_t)threadIdx.x * ST_ITEMS;
    uint64_t item[ST_ITEMS], v = 0;
    for (int k = 0; k < ST_ITEMS; ++k) {
        item[k] = i0 + k < n ? in(i0 + k) : 0;
        v += item[k];
    }
    uint64_t total;
    uint64_t run = block_scan(v, s_wave, &total) - v + (offset ? offset[blockIdx.x] : 0);
    for (int k = 0; k < ST_ITEMS; ++k) {
        if (i0 + k < n) out[i0 + k] = (TO)run;
        run += item[k];
    }
}

inline uint64_t scan_blocks(uint64_t n) { return (n + ST_B - 1) / ST_B; }

// 64-bit words of scratch scan_exclusive needs for n elements
inline uint64_t scan_scratch_words(uint64_t n) {
    uint64_t words = 0, m = scan_blocks(n) + 1;
    for (;;) {
        words += m;
        if (m <= (uint64_t)ST_B) return words;
        m = scan_blocks(m);
    }
}

// in place over m 64-bit sums; `next` = scratch behind them
void scan_sums(hipStream_t stream, uint64_t* sums, uint64_t m, uint64_t* next) {
    if (m <= (uint64_t)ST_B) {
        k_scan_down<LoadU64, uint64_t><<<1, ST_THREADS, 0, stream>>>(LoadU64{sums}, m, nullptr, sums);
        return;
    }
    const uint64_t blocks = scan_blocks(m);
    k_scan_reduce<LoadU64><<<(unsigned)blocks, ST_THREADS, 0, stream>>>(LoadU64{sums}, m, next);
    scan_sums(stream, next, blocks, next + blocks);
    k_scan_down<LoadU64, uint64_t><<<(unsigned)blocks, ST_THREADS, 0, stream>>>(LoadU64{sums}, m, next, sums);
}

// out[i] = sum of in[0 .. i) for i < n; returns where the total of all n lies (device memory, in `scratch`)
template <class L, class TO>
const uint64_t* scan_exclusive(hipStream_t stream, L in, uint64_t n, TO* out, uint64_t* scratch) {
    const uint64_t blocks = scan_blocks(n);
    // one workgroup more than the input needs: it sums nothing, and after the scan of the sums its entry is the total
    k_scan_reduce<L><<<(unsigned)(blocks + 1), ST_THREADS, 0, stream>>>(in, n, scratch);
    scan_sums(stream, scratch, blocks + 1, scratch + blocks + 1);
    if (blocks) k_scan_down<L, TO><<<(unsigned)blocks, ST_THREADS, 0, stream>>>(in, n, scratch, out);
    return scratch + blocks;
}

}  // namespace
