// The candidate finder's selection on the device (include/pepper_amd_encoder.h, pa_selector_*).
//
// replaces, for a run that opts in: the decision of pa_candidates_reference_flags + pa_candidates_select_format (candidates.cpp;
// CandidateFinder.py:356-581) over EVERY candidate row of a prediction batch on a host thread.  The decision is comparisons, one
// double division and a 20-character scan, restated here rule for rule; the record text of the rows that survive stays with
// pa_candidates_select_format, which is handed the compacted rows and keeps all of them.
//
//   name offsets   the NULs of `names` flagged and scanned (scan.h: reduce, scan of the sums, add back); NUL number k writes the
//                  start of name k + 1
//   decide         one lane per row: reference letter, low-complexity scan, allele check, rules -> keep, flags, name length;
//                  per workgroup the kept rows (ballot + popcount per wave) and the kept name bytes, wave totals through LDS
//   scan           of the workgroups' totals (both in one 64-bit word: rows << 32 | bytes)
//   compact        the same workgroups: a kept row's place is its workgroup's scanned base + the kept rows before it in the
//                  workgroup, and likewise for its name bytes -- row order, whatever the schedule
//   summary        kept rows, kept name bytes, status; name_offsets[m]
// All in one submission.  The only atomic is an OR into the status word (the cases that are handed back), whose result does not
// depend on the order; nothing on the output path is one.
//
// No fast-math flag is given to this file: the f64 division is the correctly rounded IEEE quotient the host computes, and
// the comparisons are exact.
//
// Ploidy (pa_selector_set_ploidy; pepper_amd/variant/Ploidy.py): with a haploid contig set, decide looks a row's position up in
// the contig's sorted PAR table, primes the triple of a haploid row (HET dropped, the rest renormalised by the same f64 quotient)
// and decides from the primed one; flags bit 3 says so.  compact still copies the MODEL's triple: the host formatter primes
// again from it and bit 3, so its flags remain an independent check of the device's.  No launch and no wait is added.
#include "../../include/pepper_amd.h"
#include "../../include/pepper_amd_encoder.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "kernels.h"
#include "encoder_common.h"
#include "scan.h"

namespace {

constexpr int SEL_MAX_NAME = 64;                        // a type character and at most 63 allele bytes (candidates.h: POOL_SLOT)
constexpr int64_t SEL_MAX_ROWS = 0x7fffffff;            // kept rows are numbered in int32
constexpr int64_t SEL_MAX_NAME_BYTES = 0xffffffffll;    // name starts are scanned in uint32

struct SelRegion {
    int64_t first_row, ref0, len;
    const char* ref;
};

struct LoadNul {
    const char* p;
    PA_DEV uint64_t operator()(uint64_t i) const { return p[i] == 0; }
};

PA_DEV unsigned char up(unsigned char c) { return (unsigned char)((c >= 'a' && c <= 'z') ? c - 32 : c); }
PA_DEV bool is_base(unsigned char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
PA_DEV bool is_list_byte(unsigned char c) {
    return c == ' ' || c == ',' || c == '\'' || c == '"' || c == '[' || c == ']' || c == '\n';
}

// start[k + 1] = the byte behind NUL number k (start[0] = 0 is written by thread 0); NULs past the n-th write nothing
__global__ __launch_bounds__(ST_THREADS) void k_select_name_starts(const char* __restrict__ names, uint64_t name_bytes,
                                                                   const uint32_t* __restrict__ nuls_before, int64_t n,
                                                                   uint32_t* __restrict__ start) {
    const uint64_t i = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i == 0) start[0] = 0;
    if (i >= name_bytes || names[i] != 0) return;
    const uint64_t k = nuls_before[i];
    if ((int64_t)k < n) start[k + 1] = (uint32_t)(i + 1);
}

struct DecideArgs {
    pa_candidate_rules rules;
    int64_t n;
    const int64_t* pos;
    const int32_t* depth;
    const int32_t* support;
    const float* pred;
    const char* names;
    uint64_t name_bytes;
    const uint32_t* start;            // [n + 1]
    const uint64_t* n_nuls;           // the scan's total
    const SelRegion* regions;
    int n_regions;
    uint8_t* keep_len;                // 0: not kept, else the name's bytes with its NUL
    uint8_t* flags;
    uint8_t* letter;
    uint8_t* rep;
    uint64_t* block_total;            // kept rows << 32 | kept name bytes
    uint32_t* status;
    // the ploidy of the call's one contig (pa_selector_set_ploidy): haploid 0 -> every row diploid, the table is not read
    int32_t haploid;
    int64_t n_par;
    const int64_t* par_start;         // [n_par] ascending, disjoint: the stretches that stay diploid
    const int64_t* par_end;
};

__global__ __launch_bounds__(ST_THREADS) void k_select_decide(DecideArgs a) {
    __shared__ uint32_t s_rows[ST_THREADS / 64], s_bytes[ST_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    const bool counted = *a.n_nuls == (uint64_t)a.n;    // (uniform) otherwise the name starts mean nothing: nothing is kept
    uint32_t keep_len = 0, status = 0;
    uint8_t flags = 0, letter = 0, rep = 0;
    if (i < a.n && !counted) a.keep_len[i] = 0;
    if (i < a.n && counted) {
        // the row's region: the last one that starts at or before it
        int lo = 0;
        for (int hi = a.n_regions; hi - lo > 1;) {
            const int mid = (lo + hi) >> 1;
            if (a.regions[mid].first_row <= i) lo = mid; else hi = mid;
        }
        const SelRegion reg = a.regions[lo];
        const int64_t p = a.pos[i];
        const bool inside = p >= reg.ref0 && p - reg.ref0 < reg.len;
        if (inside) {
            const int64_t q = p - reg.ref0;
            letter = up((unsigned char)reg.ref[q]);
            // the context ref[max(0, p - 10), p + 10) cut at the end of the reference; in front of reference[0] it cannot be read
            int64_t ctx_lo = (p - 10 > 0 ? p - 10 : 0) - reg.ref0;
            if (ctx_lo < 0) {
                status |= PA_SELECT_CONTEXT;
                ctx_lo = 0;
            }
            const int64_t ctx_hi = q + 10 < reg.len ? q + 10 : reg.len;
            const int64_t touch_lo = q - 5 > ctx_lo ? q - 5 : ctx_lo, touch_hi = q + 4 < ctx_hi ? q + 4 : ctx_hi;
            int64_t run_start = ctx_lo;
            unsigned char here = up((unsigned char)reg.ref[ctx_lo]);
            for (int64_t k = ctx_lo; k < ctx_hi; ++k) {
                const unsigned char next = k + 1 < ctx_hi ? up((unsigned char)reg.ref[k + 1]) : 0;
                if (k + 1 == ctx_hi || next != here) {
                    if (k + 1 - run_start >= 5 && run_start < touch_hi && k + 1 > touch_lo) rep = 1;
                    run_start = k + 1;
                }
                here = next;
            }
        }
        // the name: its bytes are looked at whatever the letter is (the host refuses a batch for any one of them)
        const uint32_t n0 = a.start[i], n1 = a.start[i + 1];
        const int64_t code_len = (int64_t)n1 - (int64_t)n0 - 1;
        bool plain = true;
        if (code_len < 1 || code_len > SEL_MAX_NAME || n1 > a.name_bytes) {
            status |= PA_SELECT_NAME;
            plain = false;
        } else {
            for (int64_t k = 0; k < code_len; ++k) {
                const unsigned char c = (unsigned char)a.names[n0 + k];
                if (is_list_byte(c)) status |= PA_SELECT_NAME;
                if (k > 0 && !is_base(c)) plain = false;
            }
        }
        if (is_base(letter) && plain) {
            const int32_t depth = a.depth[i], support = a.support[i];
            const int kind = (int)(unsigned char)a.names[n0] - '1';
            if (depth == 0) {
                status |= PA_SELECT_ZERO_DEPTH;
            } else if (kind >= 0 && kind <= 2) {
                float p0 = a.pred[3 * i], p1 = a.pred[3 * i + 1], p2 = a.pred[3 * i + 2];
                if (p0 != p0 || p1 != p1 || p2 != p2) {
                    status |= PA_SELECT_NAN;
                } else {
                    bool hap = false;
                    if (a.haploid) {                     // (uniform)
                        // haploid unless a PAR interval holds p: the last interval that starts at or before p
                        int64_t lo = 0;
                        for (int64_t hi = a.n_par; lo < hi;) {
                            const int64_t mid = (lo + hi) >> 1;
                            if (a.par_start[mid] <= p) lo = mid + 1; else hi = mid;
                        }
                        hap = !(lo > 0 && p < a.par_end[lo - 1]);
                        if (hap) {
                            // the primed triple (Ploidy.py; candidates.cpp restates it too): the rules below read it, the
                            // compaction copies the model's
                            const double s = (double)p0 + (double)p2;
                            p1 = 0.0f;
                            if (s == 0) {
                                p0 = p2 = 0.5f;
                            } else {
                                const float q0 = (float)((double)p0 / s), q2 = (float)((double)p2 / s);
                                p0 = q0;
                                p2 = q2;
                            }
                        }
                    }
                    const int g = (p1 > p0) ? ((p2 > p1) ? 2 : 1) : ((p2 > p0) ? 2 : 0);   // first maximum
                    const double non_alt = p1 > p2 ? p1 : p2;
                    const bool by_probability = non_alt >= (rep ? a.rules.p_value_in_lc[kind] : a.rules.p_value[kind]);
                    bool admitted = by_probability;
                    if (!admitted) {
                        const double above = a.rules.report_above_freq[kind];
                        admitted = 0 < above && above <= (double)support / (double)depth;
                    }
                    if (admitted) {
                        const bool swap = kind == 2 && by_probability;
                        const bool is_snp = code_len - 1 <= 1;      // max(len(REF), len(ALT)) == 1, swapped or not
                        flags = (uint8_t)((is_snp ? 1 : 0) | (swap ? 4 : 0) | (hap ? 8 : 0) | (g << 4));
                        keep_len = (uint32_t)code_len + 1;
                    }
                }
            }
        }
        a.keep_len[i] = (uint8_t)keep_len;
        a.flags[i] = flags;
        a.letter[i] = letter;
        a.rep[i] = rep;
    }
    if (status) atomicOr(a.status, status);
    // the workgroup's totals: kept rows from the ballot, kept name bytes summed over the wave, wave totals through LDS
    const unsigned long long mask = __ballot(keep_len != 0);
    uint32_t bytes = keep_len;
    for (int d = 32; d; d >>= 1) bytes += (uint32_t)__shfl_xor((int)bytes, d);
    if (lane == 0) {
        s_rows[wave] = (uint32_t)__popcll(mask);
        s_bytes[wave] = bytes;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t rows = 0, all = 0;
        for (int w = 0; w < ST_THREADS / 64; ++w) {
            rows += s_rows[w];
            all += s_bytes[w];
        }
        a.block_total[blockIdx.x] = (rows << 32) | all;
    }
}

struct CompactArgs {
    int64_t n;
    const int64_t* pos;
    const int32_t* depth;
    const int32_t* support;
    const float* pred;
    const char* names;
    const uint32_t* start;
    const uint8_t* keep_len;
    const uint8_t* flags;
    const uint8_t* letter;
    const uint8_t* rep;
    const uint64_t* block_base;       // the exclusive scan of block_total
    uint64_t name_bytes;
    int32_t* o_row;
    uint8_t* o_flags;
    uint8_t* o_letter;
    uint8_t* o_rep;
    int64_t* o_pos;
    int64_t* o_depth;
    int64_t* o_support;
    float* o_pred;
    char* o_names;
    int64_t* o_name_off;
};

__global__ __launch_bounds__(ST_THREADS) void k_select_compact(CompactArgs a) {
    __shared__ uint64_t s_wave[ST_THREADS / 64];
    const int64_t i = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    const uint32_t keep_len = i < a.n ? a.keep_len[i] : 0;
    const uint64_t mine = keep_len ? ((uint64_t)1 << 32) | keep_len : 0;
    uint64_t total;
    const uint64_t at = block_scan(mine, s_wave, &total) - mine + a.block_base[blockIdx.x];
    if (!keep_len) return;
    const uint64_t o = at >> 32, b = at & 0xffffffffull;
    if (o >= (uint64_t)a.n || b + keep_len > a.name_bytes || (uint64_t)a.start[i] + keep_len > a.name_bytes) return;      // (cannot be: the outputs have room for every row)
    a.o_row[o] = (int32_t)i;
    a.o_flags[o] = a.flags[i];
    a.o_letter[o] = a.letter[i];
    a.o_rep[o] = a.rep[i];
    a.o_pos[o] = a.pos[i];
    a.o_depth[o] = a.depth[i];
    a.o_support[o] = a.support[i];
    a.o_pred[3 * o] = a.pred[3 * i];
    a.o_pred[3 * o + 1] = a.pred[3 * i + 1];
    a.o_pred[3 * o + 2] = a.pred[3 * i + 2];
    a.o_name_off[o] = (int64_t)b;
    // one lane per name: 2 to 65 bytes, its NUL among them
    const char* src = a.names + a.start[i];
    for (uint32_t k = 0; k < keep_len; ++k) a.o_names[b + k] = src[k];
}

// words: [0] kept rows, [1] kept name bytes, [2] status
__global__ void k_select_summary(const uint64_t* __restrict__ total, const uint64_t* __restrict__ n_nuls, int64_t n,
                                 const uint32_t* __restrict__ status, int64_t* __restrict__ o_name_off, int64_t* __restrict__ words) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t rows = *total >> 32, bytes = *total & 0xffffffffull;
    words[0] = (int64_t)rows;
    words[1] = (int64_t)bytes;
    words[2] = (int64_t)(*status | (*n_nuls != (uint64_t)n ? (uint32_t)PA_SELECT_NAME_COUNT : 0u));
    if (rows <= (uint64_t)n) o_name_off[rows] = (int64_t)bytes;
}

struct Buffer {
    void* p = nullptr;
    size_t cap = 0;
    bool grow(size_t need) {
        if (need <= cap) return true;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = need + need / 8 + 4096;
        if (hipMalloc(&p, want) != hipSuccess) return false;
        cap = want;
        return true;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T> T* as() const { return (T*)p; }
};

}  // namespace

struct pa_selector {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::mutex lock;
    // a host-pointer call's uploads
    Buffer u_pos, u_depth, u_support, u_pred, u_names, u_ref;
    // tables of a run
    Buffer t_regions, t_nuls, t_start, t_scan, t_keep, t_flags, t_letter, t_rep, t_block, t_bscan, t_words;
    // the compacted rows
    Buffer o_row, o_flags, o_letter, o_rep, o_pos, o_depth, o_support, o_pred, o_names, o_name_off;
    int64_t* h_words = nullptr;       // page-locked: the summary
    bool have = false;                // a run has finished: the two below speak of it
    int64_t kept = 0, kept_bytes = 0;
    int32_t status = 0;
    // the ploidy table of the contig the runs are about (pa_selector_set_ploidy): uploaded on set, read by every run
    Buffer t_par;                     // n_par starts, then n_par ends
    int32_t haploid = 0;
    int64_t n_par = 0;
};

namespace {

#define SEL_HIP(expr)                                                                                                 \
    do {                                                                                                              \
        hipError_t e_ = (expr);                                                                                       \
        if (e_ != hipSuccess) return pa::set_error(PA_ERR_HIP, std::string("selector: " #expr ": ") + hipGetErrorString(e_)); \
    } while (0)

std::vector<Buffer*> buffers_of(pa_selector* s) {
    return {&s->u_pos, &s->u_depth, &s->u_support, &s->u_pred, &s->u_names, &s->u_ref, &s->t_regions, &s->t_nuls, &s->t_start, &s->t_scan,
            &s->t_keep, &s->t_flags, &s->t_letter, &s->t_rep, &s->t_block, &s->t_bscan, &s->t_words, &s->o_row, &s->o_flags, &s->o_letter,
            &s->o_rep, &s->o_pos, &s->o_depth, &s->o_support, &s->o_pred, &s->o_names, &s->o_name_off, &s->t_par};
}

// One run over arrays that are all in the memory of the selector's device (`regions`: host table, device references).  The
// caller holds the lock.
int select_device(pa_selector* s, const pa_candidate_rules* rules, int64_t n, const int64_t* pos, const int32_t* depth,
                  const int32_t* support, const float* pred, const char* names, int64_t name_bytes,
                  const std::vector<SelRegion>& regions, pa_selection* summary) {
    s->have = false;
    const size_t rows = (size_t)n, nb = (rows + ST_THREADS - 1) / ST_THREADS;
    const size_t bytes = (size_t)name_bytes;
    const uint64_t name_words = scan_scratch_words(bytes), block_words = scan_scratch_words(nb);
    if (!s->t_regions.grow(regions.size() * sizeof(SelRegion) + 8) || !s->t_nuls.grow(bytes * 4 + 8) || !s->t_start.grow((rows + 1) * 4) ||
        !s->t_scan.grow((name_words + block_words) * 8 + 8) || !s->t_keep.grow(rows + 8) || !s->t_flags.grow(rows + 8) ||
        !s->t_letter.grow(rows + 8) || !s->t_rep.grow(rows + 8) || !s->t_block.grow(nb * 8 + 8) || !s->t_bscan.grow(nb * 8 + 8) ||
        !s->t_words.grow(64) || !s->o_row.grow(rows * 4 + 8) || !s->o_flags.grow(rows + 8) || !s->o_letter.grow(rows + 8) ||
        !s->o_rep.grow(rows + 8) || !s->o_pos.grow(rows * 8 + 8) || !s->o_depth.grow(rows * 8 + 8) || !s->o_support.grow(rows * 8 + 8) ||
        !s->o_pred.grow(rows * 12 + 8) || !s->o_names.grow(bytes + 8) || !s->o_name_off.grow((rows + 1) * 8)) {
        (void)hipGetLastError();
        return pa::set_error(PA_ERR_HIP, "selector: no device memory for the tables of " + std::to_string(n) + " rows");
    }
    hipStream_t st = s->stream;
    uint32_t* d_status = s->t_words.as<uint32_t>();           // [0] status; the summary's three words from byte 16
    int64_t* d_words = (int64_t*)(s->t_words.as<uint8_t>() + 16);
    SEL_HIP(hipMemsetAsync(d_status, 0, 4, st));
    if (!regions.empty())
        SEL_HIP(hipMemcpyAsync(s->t_regions.p, regions.data(), regions.size() * sizeof(SelRegion), hipMemcpyHostToDevice, st));
    // 1. name offsets
    uint64_t* scratch = s->t_scan.as<uint64_t>();
    const uint64_t* d_nuls = scan_exclusive<LoadNul, uint32_t>(st, LoadNul{names}, bytes, s->t_nuls.as<uint32_t>(), scratch);
    SEL_HIP(hipGetLastError());
    k_select_name_starts<<<(unsigned)std::max<size_t>(1, (bytes + ST_THREADS - 1) / ST_THREADS), ST_THREADS, 0, st>>>(
        names, bytes, s->t_nuls.as<uint32_t>(), n, s->t_start.as<uint32_t>());
    SEL_HIP(hipGetLastError());
    // 2. decide
    if (nb) {
        DecideArgs d;
        d.rules = *rules; d.n = n; d.pos = pos; d.depth = depth; d.support = support; d.pred = pred; d.names = names;
        d.name_bytes = bytes; d.start = s->t_start.as<uint32_t>(); d.n_nuls = d_nuls; d.regions = s->t_regions.as<SelRegion>();
        d.n_regions = (int)regions.size(); d.keep_len = s->t_keep.as<uint8_t>(); d.flags = s->t_flags.as<uint8_t>();
        d.letter = s->t_letter.as<uint8_t>(); d.rep = s->t_rep.as<uint8_t>(); d.block_total = s->t_block.as<uint64_t>();
        d.status = d_status;
        d.haploid = s->haploid; d.n_par = s->haploid ? s->n_par : 0;
        d.par_start = s->t_par.as<int64_t>(); d.par_end = s->t_par.as<int64_t>() + d.n_par;
        k_select_decide<<<(unsigned)nb, ST_THREADS, 0, st>>>(d);
        SEL_HIP(hipGetLastError());
    }
    // 3. the workgroups' bases
    const uint64_t* d_total = scan_exclusive<LoadU64, uint64_t>(st, LoadU64{s->t_block.as<uint64_t>()}, nb, s->t_bscan.as<uint64_t>(),
                                                                scratch + name_words);
    SEL_HIP(hipGetLastError());
    // 4. compact
    if (nb) {
        CompactArgs c;
        c.n = n; c.pos = pos; c.depth = depth; c.support = support; c.pred = pred; c.names = names; c.start = s->t_start.as<uint32_t>();
        c.keep_len = s->t_keep.as<uint8_t>(); c.flags = s->t_flags.as<uint8_t>(); c.letter = s->t_letter.as<uint8_t>();
        c.rep = s->t_rep.as<uint8_t>(); c.block_base = s->t_bscan.as<uint64_t>(); c.name_bytes = bytes;
        c.o_row = s->o_row.as<int32_t>(); c.o_flags = s->o_flags.as<uint8_t>(); c.o_letter = s->o_letter.as<uint8_t>();
        c.o_rep = s->o_rep.as<uint8_t>(); c.o_pos = s->o_pos.as<int64_t>(); c.o_depth = s->o_depth.as<int64_t>();
        c.o_support = s->o_support.as<int64_t>(); c.o_pred = s->o_pred.as<float>(); c.o_names = s->o_names.as<char>();
        c.o_name_off = s->o_name_off.as<int64_t>();
        k_select_compact<<<(unsigned)nb, ST_THREADS, 0, st>>>(c);
        SEL_HIP(hipGetLastError());
    }
    // 5. summary
    k_select_summary<<<1, 64, 0, st>>>(d_total, d_nuls, n, d_status, s->o_name_off.as<int64_t>(), d_words);
    SEL_HIP(hipGetLastError());
    SEL_HIP(hipMemcpyAsync(s->h_words, d_words, 24, hipMemcpyDeviceToHost, st));
    SEL_HIP(hipStreamSynchronize(st));
    s->kept = s->h_words[0];
    s->kept_bytes = s->h_words[1];
    s->status = (int32_t)s->h_words[2];
    s->have = true;
    summary->kept_rows = s->status ? 0 : s->kept;
    summary->kept_name_bytes = s->status ? 0 : s->kept_bytes;
    summary->status = s->status;
    summary->reserved = 0;
    return PA_OK;
}

}  // namespace

extern "C" {

int pa_selector_limits(int64_t* out, int32_t n) {
    if (!out || n < 0) return pa::set_error(PA_ERR_INVALID, "selector limits: null or negative argument");
    const int64_t v[5] = {ST_THREADS, ST_B, SEL_MAX_NAME, (int64_t)ST_B * (ST_B - 1), SEL_MAX_ROWS};
    for (int32_t i = 0; i < n; ++i) out[i] = i < 5 ? v[i] : 0;
    return PA_OK;
}

int pa_selector_create(int32_t device, void* hip_stream, pa_selector** out) {
    if (!out) return pa::set_error(PA_ERR_INVALID, "selector: null argument");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return pa::set_error(PA_ERR_NO_DEVICE, "no HIP device visible: the device selection has no CPU fallback "
                                               "(pa_candidates_select_format is the host form)");
    if (device < 0 || device >= count) return pa::set_error(PA_ERR_INVALID, "selector: device ordinal out of range");
    SEL_HIP(hipSetDevice(device));
    auto* s = new pa_selector();
    s->device = device;
    s->stream = (hipStream_t)hip_stream;
    if (!hip_stream) {
        if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
            delete s;
            return pa::set_error(PA_ERR_HIP, "selector: stream creation failed");
        }
        s->own_stream = true;
    }
    if (hipHostMalloc((void**)&s->h_words, 64, hipHostMallocDefault) != hipSuccess) {
        if (s->own_stream) (void)hipStreamDestroy(s->stream);
        delete s;
        return pa::set_error(PA_ERR_HIP, "selector: no page-locked memory for the summary");
    }
    *out = s;
    return PA_OK;
}

void pa_selector_destroy(pa_selector* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    for (Buffer* b : buffers_of(s)) b->release();
    if (s->h_words) (void)hipHostFree(s->h_words);
    if (s->own_stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

int pa_selector_run(pa_selector* s, const pa_candidate_rules* rules, int64_t n, const int64_t* position, const int32_t* depth,
                    const int32_t* support, const float* prediction, const char* names, int64_t name_bytes, int32_t n_regions,
                    const pa_selector_region* regions, int32_t on_device, pa_selection* summary) {
    if (!s || !rules || !summary || n < 0 || name_bytes < 0 || n_regions < 0)
        return pa::set_error(PA_ERR_INVALID, "selector run: null or negative argument");
    if (n > 0 && (!position || !depth || !support || !prediction || !regions || n_regions == 0))
        return pa::set_error(PA_ERR_INVALID, "selector run: rows without their arrays or without a region");
    if (name_bytes > 0 && !names) return pa::set_error(PA_ERR_INVALID, "selector run: name bytes without names");
    if (n > SEL_MAX_ROWS || name_bytes > SEL_MAX_NAME_BYTES)
        return pa::set_error(PA_ERR_UNSUPPORTED, "selector run: more than 2^31 - 1 rows or 2^32 - 1 name bytes in one call");
    int64_t ref_total = 0;
    for (int32_t r = 0; r < n_regions; ++r) {
        const pa_selector_region& g = regions[r];
        if (g.reference_len < 0 || g.reference_start < 0 || (g.reference_len > 0 && !g.reference) ||
            (r == 0 ? g.first_row != 0 : g.first_row < regions[r - 1].first_row))
            return pa::set_error(PA_ERR_INVALID, "selector run: region " + std::to_string(r) + ": a negative length or start, a null reference, "
                                                     "or first rows that do not ascend from 0");
        ref_total += g.reference_len;
    }
    std::lock_guard<std::mutex> guard(s->lock);
    SEL_HIP(hipSetDevice(s->device));
    std::vector<SelRegion> table((size_t)n_regions);
    const size_t rows = (size_t)n;
    if (!on_device) {
        if (!s->u_pos.grow(rows * 8 + 8) || !s->u_depth.grow(rows * 4 + 8) || !s->u_support.grow(rows * 4 + 8) || !s->u_pred.grow(rows * 12 + 8) ||
            !s->u_names.grow((size_t)name_bytes + 8) || !s->u_ref.grow((size_t)ref_total + 8)) {
            (void)hipGetLastError();
            return pa::set_error(PA_ERR_HIP, "selector run: no device memory for the uploads");
        }
        hipStream_t st = s->stream;
        if (rows) {
            SEL_HIP(hipMemcpyAsync(s->u_pos.p, position, rows * 8, hipMemcpyHostToDevice, st));
            SEL_HIP(hipMemcpyAsync(s->u_depth.p, depth, rows * 4, hipMemcpyHostToDevice, st));
            SEL_HIP(hipMemcpyAsync(s->u_support.p, support, rows * 4, hipMemcpyHostToDevice, st));
            SEL_HIP(hipMemcpyAsync(s->u_pred.p, prediction, rows * 12, hipMemcpyHostToDevice, st));
        }
        if (name_bytes) SEL_HIP(hipMemcpyAsync(s->u_names.p, names, (size_t)name_bytes, hipMemcpyHostToDevice, st));
        int64_t at = 0;
        for (int32_t r = 0; r < n_regions; ++r) {
            const pa_selector_region& g = regions[r];
            if (g.reference_len) SEL_HIP(hipMemcpyAsync(s->u_ref.as<char>() + at, g.reference, (size_t)g.reference_len, hipMemcpyHostToDevice, st));
            table[(size_t)r] = SelRegion{g.first_row, g.reference_start, g.reference_len, s->u_ref.as<char>() + at};
            at += g.reference_len;
        }
        return select_device(s, rules, n, s->u_pos.as<int64_t>(), s->u_depth.as<int32_t>(), s->u_support.as<int32_t>(), s->u_pred.as<float>(),
                             s->u_names.as<char>(), name_bytes, table, summary);
    }
    for (int32_t r = 0; r < n_regions; ++r)
        table[(size_t)r] = SelRegion{regions[r].first_row, regions[r].reference_start, regions[r].reference_len, regions[r].reference};
    return select_device(s, rules, n, position, depth, support, prediction, names, name_bytes, table, summary);
}

int pa_selector_set_ploidy(pa_selector* s, int32_t haploid_contig, int64_t n_par, const int64_t* par_start, const int64_t* par_end) {
    if (!s || n_par < 0 || (n_par > 0 && (!par_start || !par_end)))
        return pa::set_error(PA_ERR_INVALID, "selector set ploidy: null or negative argument");
    if (!haploid_contig && n_par > 0)
        return pa::set_error(PA_ERR_INVALID, "selector set ploidy: PAR intervals on a contig that is not haploid");
    for (int64_t k = 0; k < n_par; ++k)
        if (par_start[k] < 0 || par_end[k] <= par_start[k] || (k > 0 && par_start[k] < par_end[k - 1]))
            return pa::set_error(PA_ERR_INVALID, "selector set ploidy: interval " + std::to_string(k) + " is empty, negative or not behind "
                                                     "the one before it");
    std::lock_guard<std::mutex> guard(s->lock);
    SEL_HIP(hipSetDevice(s->device));
    s->haploid = 0;                   // (a failed upload leaves the selector diploid, not with half a table)
    s->n_par = 0;
    if (haploid_contig && n_par > 0) {
        const size_t bytes = (size_t)n_par * 8;
        if (!s->t_par.grow(2 * bytes + 8)) {
            (void)hipGetLastError();
            return pa::set_error(PA_ERR_HIP, "selector set ploidy: no device memory for " + std::to_string(n_par) + " intervals");
        }
        // behind the runs already on the stream, and complete before the caller's arrays may go away
        SEL_HIP(hipMemcpyAsync(s->t_par.p, par_start, bytes, hipMemcpyHostToDevice, s->stream));
        SEL_HIP(hipMemcpyAsync(s->t_par.as<uint8_t>() + bytes, par_end, bytes, hipMemcpyHostToDevice, s->stream));
        SEL_HIP(hipStreamSynchronize(s->stream));
        s->n_par = n_par;
    }
    s->haploid = haploid_contig ? 1 : 0;
    return PA_OK;
}

int pa_selector_take(pa_selector* s, int32_t* row, uint8_t* flags, uint8_t* letter, uint8_t* in_repeat, int64_t* position,
                     int64_t* depth, int64_t* support, float* prediction, char* names, int64_t* name_offsets) {
    if (!s) return pa::set_error(PA_ERR_INVALID, "selector take: null handle");
    std::lock_guard<std::mutex> guard(s->lock);
    if (!s->have) return pa::set_error(PA_ERR_INVALID, "selector take: no run has finished");
    if (s->status)
        return pa::set_error(PA_ERR_INVALID, "selector take: the last run was handed back (status " + std::to_string(s->status) +
                                                 "): its rows are selected on the host");
    SEL_HIP(hipSetDevice(s->device));
    const size_t m = (size_t)s->kept;
    hipStream_t st = s->stream;
    if (m) {
        if (row) SEL_HIP(hipMemcpyAsync(row, s->o_row.p, m * 4, hipMemcpyDeviceToHost, st));
        if (flags) SEL_HIP(hipMemcpyAsync(flags, s->o_flags.p, m, hipMemcpyDeviceToHost, st));
        if (letter) SEL_HIP(hipMemcpyAsync(letter, s->o_letter.p, m, hipMemcpyDeviceToHost, st));
        if (in_repeat) SEL_HIP(hipMemcpyAsync(in_repeat, s->o_rep.p, m, hipMemcpyDeviceToHost, st));
        if (position) SEL_HIP(hipMemcpyAsync(position, s->o_pos.p, m * 8, hipMemcpyDeviceToHost, st));
        if (depth) SEL_HIP(hipMemcpyAsync(depth, s->o_depth.p, m * 8, hipMemcpyDeviceToHost, st));
        if (support) SEL_HIP(hipMemcpyAsync(support, s->o_support.p, m * 8, hipMemcpyDeviceToHost, st));
        if (prediction) SEL_HIP(hipMemcpyAsync(prediction, s->o_pred.p, m * 12, hipMemcpyDeviceToHost, st));
        if (names && s->kept_bytes) SEL_HIP(hipMemcpyAsync(names, s->o_names.p, (size_t)s->kept_bytes, hipMemcpyDeviceToHost, st));
    }
    if (name_offsets) SEL_HIP(hipMemcpyAsync(name_offsets, s->o_name_off.p, (m + 1) * 8, hipMemcpyDeviceToHost, st));
    SEL_HIP(hipStreamSynchronize(st));
    return PA_OK;
}

int pa_encoder_select_candidates(pa_encoder* e, pa_selector* s, const float* prediction, const pa_candidate_rules* rules,
                                 pa_selection* summary) {
    if (!e || !s || !rules || !summary) return pa::set_error(PA_ERR_INVALID, "select candidates: null argument");
    std::lock_guard<std::mutex> guard(s->lock);
    SEL_HIP(hipSetDevice(s->device));
    pa_enc::SelectionView v;
    const int rc = pa_enc::selection_view(e, s->device, s->stream, &v);
    if (rc != PA_OK) return rc;
    if (v.n > 0 && !prediction) return pa::set_error(PA_ERR_INVALID, "select candidates: rows without probabilities");
    std::vector<SelRegion> table(v.regions.size());
    for (size_t r = 0; r < table.size(); ++r)
        table[r] = SelRegion{v.regions[r].first_row, v.regions[r].reference_start, v.regions[r].reference_len, v.regions[r].reference};
    return select_device(s, rules, v.n, v.positions, v.depths, v.supports, prediction, v.names, v.name_bytes, table, summary);
}

}  // extern "C"
