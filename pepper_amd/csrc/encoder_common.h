// Shared pieces of the two summary encoders (encoder.hip: variant, encoder_polish.hip: polish).
//
// Both walk CIGAR strings on the device the same way.  A wave takes 64 operations at a time, one per lane; a wave-wide
// prefix sum of the reference / read advances gives every operation its first reference row and its first read index
// (no serial walk); the sparse per-operation work (insert anchors, deletion anchors) is done one operation per lane, the
// dense per-base work one REFERENCE ROW per lane: lane l takes row span_lo + l + 64 k and finds the operation that owns
// it by a 6-step binary search over the 64 first-rows the wave has just written to its LDS scratch.  Consecutive lanes
// therefore touch consecutive rows (conflict-free LDS atomics on a [counter][row] tile) and consecutive read bytes
// (coalesced loads), whatever the lengths of the match runs -- a lane-per-operation walk idles on the longest run of the 64,
// a wave-per-operation walk (round 2) used 10-20 lanes of 64 on nanopore CIGARs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/pepper_amd.h"
#include "../../include/pepper_amd_encoder.h"
#include "kernels.h"

namespace pa_enc {

enum { OP_M = 0, OP_I = 1, OP_D = 2, OP_N = 3, OP_S = 4, OP_H = 5, OP_P = 6, OP_EQ = 7, OP_X = 8 };

// inclusive prefix sum over the 64 lanes of a wave on the DPP network (row_shr 1/2/4/8 inside each row of 16 lanes, then
// row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3); lanes without a source add the `old` operand, 0
__device__ __forceinline__ int wave_inclusive_sum(int x) {
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);
    return x;
}
__device__ __forceinline__ int wave_total(int inclusive) { return __builtin_amdgcn_readlane(inclusive, 63); }
__device__ __forceinline__ int wave_sum(int x) { return wave_total(wave_inclusive_sum(x)); }
// minimum / maximum over the wave on the same network (identity in the lanes without a source), the same in every lane
__device__ __forceinline__ int wave_min(int x) {
    const int id = 0x7fffffff;
    x = min(x, __builtin_amdgcn_update_dpp(id, x, 0x111, 0xf, 0xf, false));
    x = min(x, __builtin_amdgcn_update_dpp(id, x, 0x112, 0xf, 0xf, false));
    x = min(x, __builtin_amdgcn_update_dpp(id, x, 0x114, 0xf, 0xf, false));
    x = min(x, __builtin_amdgcn_update_dpp(id, x, 0x118, 0xf, 0xf, false));
    x = min(x, __builtin_amdgcn_update_dpp(id, x, 0x142, 0xa, 0xf, false));
    x = min(x, __builtin_amdgcn_update_dpp(id, x, 0x143, 0xc, 0xf, false));
    return __builtin_amdgcn_readlane(x, 63);
}
__device__ __forceinline__ int wave_max(int x) { return -wave_min(-x); }       // (callers keep |x| < 2^31 - 1)

// reference / read advance of one operation as populate_summary_matrix steps (region_summary.cpp:357-563): N and P advance
// the reference AND, through the missing break, the read (:556-561)
__device__ __forceinline__ int variant_ref_advance(int op, int len) {
    return (op == OP_M || op == OP_EQ || op == OP_X || op == OP_D || op == OP_N || op == OP_P) ? len : 0;
}
__device__ __forceinline__ int variant_read_advance(int op, int len) {
    return (op == OP_M || op == OP_EQ || op == OP_X || op == OP_I || op == OP_S || op == OP_N || op == OP_P) ? len : 0;
}
// the polish walk (summary_generator.cpp:47-121): D, N and P are gaps that advance only the reference
__device__ __forceinline__ int polish_ref_advance(int op, int len) {
    return (op == OP_M || op == OP_EQ || op == OP_X || op == OP_D || op == OP_N || op == OP_P) ? len : 0;
}
__device__ __forceinline__ int polish_read_advance(int op, int len) {
    return (op == OP_M || op == OP_EQ || op == OP_X || op == OP_I || op == OP_S) ? len : 0;
}

// last j in [0, 64) with first_row[j] <= row; first_row is non-decreasing (INT_MAX past the read's last operation) and
// first_row[0] <= row
__device__ __forceinline__ int owner_of_row(const int* first_row, int row) {
    int j = 0;
#pragma unroll
    for (int step = 32; step > 0; step >>= 1)
        if (first_row[j + step] <= row) j += step;
    return j;
}

struct DBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool ensure(size_t need) {
        if (need <= bytes) return true;
        static const bool trace = getenv("PA_TRACE_ALLOC") != nullptr;      // every (re)allocation on stderr: a hipFree waits for the device
        if (trace) fprintf(stderr, "[alloc] device buffer %zu -> %zu bytes\n", bytes, need + need / 4 + 256);
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        const size_t grow = need + need / 4 + 256;
        if (hipMalloc(&p, grow) != hipSuccess) return false;
        bytes = grow;
        return true;
    }
    template <typename T> T* as() const { return static_cast<T*>(p); }
    ~DBuf() { if (p) (void)hipFree(p); }
};

// page-locked host buffer that only grows (results of a run: one asynchronous copy each, no page faults per run)
struct HBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool ensure(size_t need) {
        if (need <= bytes) return true;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
        const size_t grow = need + need / 2 + 4096;
        if (hipHostMalloc(&p, grow, hipHostMallocDefault) != hipSuccess) return false;
        bytes = grow;
        return true;
    }
    template <typename T> T* as() const { return static_cast<T*>(p); }
    ~HBuf() { if (p) (void)hipHostFree(p); }
};


// one read of a batch: where its bases, qualities and operations start in the concatenated device arrays
struct ReadRec {
    int64_t s0;        // first base in seq / qual
    int32_t c0;        // first operation in cigar_op / cigar_len
    int32_t ncig;
    int32_t slen;
    int32_t row0;      // type_read.pos - region_start
    int32_t region;
    int32_t flags;     // 1 reverse strand, 2 mapping quality > 0
};
constexpr int READ_REV = 1, READ_MAPQ_OK = 2;

}  // namespace pa_enc

#define ENC_HIP(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return pa::set_error(PA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define ENC_ALLOC(buf, bytes_)                                                                          \
    do {                                                                                                \
        if (!(buf).ensure(bytes_)) return pa::set_error(PA_ERR_HIP, "hipMalloc failed in encoder workspace"); \
    } while (0)

// The reservoir sample of deep intervals (pa_encoder_set_sampling; reservoir_keep_kernel in encoder.hip): the handle's
// setting, its counters and the small tables of a launch.
struct pa_sampler {
    bool on = false;
    uint32_t seed = 0;
    int32_t cap = 0;                 // MAX_READS_IN_REGION of the caller
    double rate = 1.0;               // downsample_rate (polish: 1.0)
    int64_t regions = 0, dropped = 0;     // intervals sampled / reads dropped since the handle was created
    int pending = 0;                 // intervals of the last launch whose {n, kept} have not been added to the counters yet
    pa_enc::DBuf d_tab, d_keep;      // [SampRec x c][int2 x c] | one byte per (interval, rank): in a slot
    pa_enc::HBuf h_tab;
};

// The setting of a per-position track of the variant encoder (encoder.hip: depth classes, reference blocks).
struct pa_track_setting {
    int32_t n = 0;                   // classes (0: the track is off) ...
    int32_t lower[8] = {};           // ... and their ascending lower bounds, lower[0] == 0
    int64_t cap = 0;                 // the track's debug capacity from the environment, as the setting call read it (0: sized by the batch)
    void set(int32_t n_classes, const int32_t* bounds, const char* cap_env) {
        n = n_classes;
        for (int32_t k = 0; k < 8; ++k) lower[k] = k < n ? bounds[k] : 0;
        const char* text = n > 0 ? getenv(cap_env) : nullptr;
        cap = text ? std::max<int64_t>(0, atoll(text)) : 0;
    }
};

struct pa_variant_batch;     // encoder.hip
struct pa_polish_batch;      // encoder_polish.hip

struct pa_encoder {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev[16] = {};                        // ([12], [13]: around the depth-run kernels; [14], [15]: around the reference-block kernels)
    pa_variant_batch* variant = nullptr;
    pa_polish_batch* polish = nullptr;
    struct pa_realigner* realigner = nullptr;      // the polish image chain's re-aligner on this encoder's stream (made on first use)
    pa_sampler sampler;
    bool split_walk = false;                       // pa_encoder_set_split_slices: the record walk resolves CIGARs kept in the CG tag
    int64_t n_targets = 0;                         // pa_encoder_set_targets: intervals of the table (0: no restriction) ...
    pa_enc::DBuf d_target_table;                   // ... [start x n][end x n] on the device
    pa_track_setting depth_bins;                   // pa_encoder_set_depth_bins: the bins of the depth classes (cap: PEPPER_AMD_DEPTH_RUN_CAP)
    pa_track_setting ref_bands;                    // pa_encoder_set_ref_confidence: the GQ bands of the reference blocks (cap: PEPPER_AMD_REF_BLOCK_CAP) ...
    pa_enc::DBuf d_gq_table;                       // ... and the 101 x 101 uint8 table [n_ref][n_alt] -> GQ on the device
    std::vector<int64_t> seq_off;                  // pa_encoder_set_seq_offsets: per packed read of the NEXT staging where its bases lie (-1: behind its operations)
};

// ---- the polish image chain (encoder_polish.hip: pa_polish_chain_*) crosses the three files; the pieces it calls --------------
namespace pa_enc {
// what unpack_clip_kernel (encoder.hip) left ON THE DEVICE for the (read, region) pairs of a packed batch: every pair's clipped
// read as the host-clipped form would have uploaded it (ReadRec, CIGAR arrays, bases as text).  The CIGAR arrays have room
// for extra_ops more operations behind the total_ops the pairs may use (the re-aligned CIGARs go there): total_bases +
// n_pairs x extra_ops_per_pair of them (extra_ops_per_pair < 0: none).
struct UnpackedReads {
    ReadRec* reads = nullptr;
    int32_t* cigar_op = nullptr;
    int32_t* cigar_len = nullptr;
    const char* seq = nullptr;
    int64_t n_pairs = 0, total_bases = 0, total_ops = 0, extra_ops = 0;      // slots the pairs were given (bounds of what they use)
    int* d_live = nullptr;           // the same three on the device
    const int* h_live = nullptr;     // page-locked [n_regions + 2], valid once the stream has been waited for: reads with a base
                                     // inside each region | first inconsistent read + 1 | first unsupported read + 1
};
int unpack_packed_regions(pa_encoder* e, int32_t n_regions, const int64_t* region_start, const int64_t* region_end,
                          const uint8_t* arena, int64_t arena_bytes, const pa_packed_read* reads, int32_t n_reads,
                          const int32_t* pair_read, const int32_t* region_pairs, int32_t extra_ops_per_pair, UnpackedReads* out);
// The reservoir sample over the pairs unpack_clip_kernel has just clipped (same stream, nothing waits): one workgroup of
// reservoir_keep_kernel per interval that can need it -- none, and no launch, when sampling is off or (rate >= 1 and every
// interval has at most `cap` pairs).  It clears the pairs that fall out of the sample the way the clip kernel marks a pair
// without a base inside, sets d_live[r] to the kept count and copies d_live to h_live again.  sample_collect: once the stream
// has been waited for, the launch's counts into the handle's counters.
int sample_pairs(pa_encoder* e, int32_t n_regions, const int32_t* region_pairs, ReadRec* d_reads, int* d_live, int* h_live);
void sample_collect(pa_encoder* e);
}  // namespace pa_enc

namespace pa_enc {
// What the candidate selection (select.hip: pa_encoder_select_candidates) reads of the encoder's last variant run, all of it in
// device memory: the lists where the device enumeration left them -- a host-enumerated run's lists are uploaded on `stream`
// first, once per run --, the references of the staged batch, and per region its first row (from the counts the run's one wait
// brought back: nothing is downloaded here).
struct SelectionRegion { int64_t first_row, reference_start, reference_len; const char* reference; };
struct SelectionView {
    int64_t n = 0, name_bytes = 0;
    const int64_t* positions = nullptr;
    const int32_t* depths = nullptr;
    const int32_t* supports = nullptr;
    const char* names = nullptr;
    std::vector<SelectionRegion> regions;
};
int selection_view(pa_encoder* e, int device, hipStream_t stream, SelectionView* out);
}  // namespace pa_enc

namespace pa_ra {
// The re-aligner over reads that are already on the device (realign.hip).  reads[k] (ReadRec of pair k: s0, slen, row0 = read
// position - region start, region, flags) against window `region`: codes [window_off[region], + window_len[region]) of the
// window text uploaded by this call.  Reads without READ_MAPQ_OK are not aligned (the summary skips them).  On return the
// re-aligner's stream (the one it was created on) has been waited for once or more; the results are on the device: jobs (the kernels' table: state, ref_begin, ops_off,
// n_ops per read) and the compacted operations (len << 4 | op).  d_cigar_op / d_cigar_len: the reads' clipped BAM alignments
// (ReadRec.c0 / ncig; null: none) -- only used to prove that a read's 8-bit score pass overflows, which is then not run.
struct DeviceResult {
    const void* jobs = nullptr;          // Job [n_reads] (realign.hip)
    const uint32_t* ops = nullptr;
    int64_t ops_written = 0;
    int32_t n_aligned = 0;
    int32_t n_proven = 0;                // reads whose 8-bit score pass was proven to overflow from their BAM alignment and not run
};
int align_device(pa_realigner* r, const char* window_text, int64_t window_bytes, const int64_t* window_off,
                 const int32_t* window_len, int32_t n_windows, const pa_enc::ReadRec* d_reads, int32_t n_reads, const char* d_seq,
                 int64_t seq_bytes, int32_t max_region_len, const int32_t* d_cigar_op, const int32_t* d_cigar_len, DeviceResult* out);
// per read k with a new alignment: reads[k].row0 += ref_begin, its CIGAR = the operations decoded into cigar_op / cigar_len at
// ops_base + ops_off ('=' and 'X' as MATCH when collapse_eqx), c0 / ncig pointing there
int apply_device(pa_realigner* r, pa_enc::ReadRec* d_reads, int32_t n_reads, int32_t* cigar_op,
                 int32_t* cigar_len, int64_t ops_base, int32_t collapse_eqx);
}  // namespace pa_ra

// the two halves free their own state (defined next to the structs)
void pa_variant_batch_free(pa_variant_batch*);
void pa_polish_batch_free(pa_polish_batch*);
