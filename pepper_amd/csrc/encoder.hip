// Variant summary encoder (include/pepper_amd_encoder.h): pileups of many regions -> candidate images, one launch set.
//
// Split of the reference's RegionalSummaryGenerator::generate_summary
// (/root/reference/pepper_variant/modules/cpp/region_summary.cpp:337-916):
//   GPU   segment_reads_kernel   one wave per read: prefix sums over its CIGAR operations, one 16-byte record per
//                                (read, 512-row tile) the read touches = where the walk of that tile starts
//         tile_offsets_kernel    (run twice around an exclusive scan: count per tile, then fill each tile's slice)
//         tile_count_kernel      ONE WORKGROUP OWNS ONE TILE: 28 int32 counters x 512 rows privatised in LDS (coverage,
//                                SNP / insert / delete counts, the 16 image columns the walk updates, the 8 SNP allele
//                                tallies); its waves walk the tile's records (encoder_common.h: one row per lane, LDS
//                                atomics only, :366-551); then the same workgroup applies the per-position pass of :568-654
//                                (fractions vs thresholds in fp64, passing-site records, clamp of columns 11..24) and
//                                stores the finished tile ONCE, coalesced: int32 [row][26], the algorithmic 104 bytes per
//                                position.  No global atomics on the matrix, no zero-fill pass, no read-modify-write pass
//                                [HBM bound: 2 B per aligned base in, 104 B per position out]
//         compact_votes_kernel   indel allele votes of the sites that passed (a few per cent of all votes)
//   host  what needs strings: ordered per-site maps of allele keys for the passing sites, candidate enumeration in the
//         reference's std::set order with its filters (:669-712)
//   GPU   gather_windows_kernel  33 x 26 window copy + candidate-specific overwrite (:828-905), int32 image_matrix and
//                                the int8 wrap DataStore.py:68 applies
// Round 2 walked one wave per read with global int32 atomics on a [L+1][32] matrix: 559 MB of atomic write traffic for
// 22 MB of algorithmic bytes on one 100 kb / 60x region, 759 waves on a 1024-SIMD chip.  Here parallelism = tiles
// (~200 per 100 kb region, x regions per batch) and every matrix byte is written exactly once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pepper_amd_realign.h"
#include "encoder_common.h"
#include "candidates.h"
#include "reservoir.h"
#include "pack_rule.h"

using namespace pa_enc;
using pa_cand::SiteRec; using pa_cand::Vote; using pa_cand::CandDesc; using pa_cand::Tally; using pa_cand::AlleleSrc;
using pa_cand::is_acgt; using pa_cand::up; using pa_cand::symbol_column; using pa_cand::base_code;

namespace {

constexpr int MAXC = pa_cand::MAXC;
constexpr int TP = 512;             // rows per tile = threads of a tile_count_kernel workgroup
constexpr int MATF = 26;            // int32 per matrix row in HBM (the image columns)
constexpr int NCNT = 28;            // privatised counters per row
constexpr int NW = 8, NT = 64 * NW;  // waves / threads of a tile_count_kernel workgroup: NT == TP, a thread owns a row in the per-position pass
constexpr int UNR = 8;              // rows per lane in flight in the row phase: 64 x UNR = TP
constexpr int VCAP = 512;           // indel votes a tile keeps in LDS (nanopore: ~600 per 512 rows x 60 reads; more spill to the global list)
constexpr int XQ = 128;             // per-wave queue of the bases that are not clean matches (processed 64 at a time)
static_assert(NT == TP && 64 * UNR == TP, "one thread per row, UNR rows per lane");
static_assert(VCAP == NT, "the flush takes one buffered vote per thread");
// counter slots: 0 coverage, 1 snp_count, 2 insert_count, 3 delete_count, 4 = column 4 (forward strand coverage),
// 5..11 = columns 8..14 (forward A C G T I D *), 12 = column 15 (reverse strand coverage), 13..19 = columns 19..25,
// 20..23 / 24..27 = forward / reverse tallies of mismatching A C G T (the SNP allele map of :409-425)
enum { K_COV = 0, K_SNP = 1, K_INS = 2, K_DEL = 3, K_FWD = 4, K_REV = 12, K_TAB = 20 };
// counters of a run
enum { CT_OVF = 0, CT_VOTES = 2, CT_ERR = 3, CT_POOL = 4, CT_N = 8 };
constexpr int POOL_SLOT = pa_cand::POOL_SLOT;
// per region, behind them: [2 r] passing sites, [2 r + 1] votes of passing sites -- both lists are written region by region
// (sites of region r from row_base, votes from vote_base), so the host never has to sort a batch's records by region

struct RegRec {                      // one region of the batch, as the kernels see it
    int64_t ref_off;                 // first byte of its reference in d_ref
    int64_t row_base;                // first row of its matrix (multiple of 16: line-aligned tile stores)
    int64_t seq_base;                // first base of its reads in d_seq / d_qual
    int64_t region_start;            // contig position of row 0 (target_rows_kernel)
    int32_t ref_len, L;              // L = region_end - region_start + 1; the matrix has L + 1 rows (row L stays zero)
    int32_t tile0, n_tiles;
    int32_t cand_lo, cand_hi;        // candidate_region_start / _end as rows (clamped into int32)
    int32_t qmin;                    // smallest integer base quality that is >= min_snp_baseq (256: none)
    int32_t vote_base;               // first slot of the region's slice of the passing-vote list (= its first CIGAR operation)
    double min_snp_q, min_indel_q, snp_thr, ins_thr, del_thr, min_cov;
};
struct TileRec { int32_t read, op, row, ri; };   // walk of `read` enters the tile at operation `op`, whose first row / read index are given
// SiteRec, Vote, CandDesc: candidates.h

__device__ __forceinline__ int column_slot(int col) { return col < 15 ? col - 3 : col - 6; }   // columns 8..14 / 19..25

// ---- records: where the walk of each (read, tile) starts -----------------------------------------------------------
// Two passes of the same walk: FILL = false counts the records of every tile (atomics spread over the tiles), an exclusive
// scan turns the counts into offsets, FILL = true writes each record into its tile's slice.  (One pass appending to a
// global list cost 3 ms for 64 regions: ~300 k returning atomics on ONE counter serialise at ~10 ns each.)
template <bool FILL>
__global__ __launch_bounds__(256) void segment_reads_kernel(const ReadRec* __restrict__ reads, int n_reads,
                                                            const RegRec* __restrict__ regions,
                                                            const int32_t* __restrict__ cigar_op,
                                                            const int32_t* __restrict__ cigar_len, int* __restrict__ tile_count,
                                                            const int* __restrict__ tile_off, int* __restrict__ tile_fill,
                                                            TileRec* __restrict__ recs, int rec_cap) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_reads) return;
    const ReadRec rd = reads[r];
    if (!(rd.flags & READ_MAPQ_OK)) return;
    const RegRec* reg = regions + rd.region;
    const int L = reg->L, tile0 = reg->tile0;
    auto put = [&](int tile, int op, int row, int ri) {
        if (!FILL) {
            atomicAdd(&tile_count[tile], 1);
        } else {
            const int slot = tile_off[tile] + atomicAdd(&tile_fill[tile], 1);
            if (slot < rec_cap) recs[slot] = TileRec{r, op, row, ri};     // past the capacity: the host repeats the run with room
        }
    };
    int pos = rd.row0, ri = 0;
    if (pos > L - 1) return;
    if (pos >= 0 && lane == 0) {
        put(tile0 + pos / TP, rd.c0, pos, 0);
        // an insert in front of the read's first aligned base (S I M) is anchored on the row before it: when that row is the
        // last one of the previous tile, that tile walks the read's leading operations too
        if (pos > 0 && pos % TP == 0) put(tile0 + pos / TP - 1, rd.c0, pos, 0);
    }
    for (int cb = 0; cb < rd.ncig; cb += 64) {
        const int i = cb + lane;
        const bool valid = i < rd.ncig;
        const int op = valid ? cigar_op[rd.c0 + i] : OP_H;
        const int len = valid ? cigar_len[rd.c0 + i] : 0;
        const int radv = variant_ref_advance(op, len), qadv = variant_read_advance(op, len);
        const int rinc = wave_inclusive_sum(radv), qinc = FILL ? wave_inclusive_sum(qadv) : 0;
        const int first = pos + rinc - radv, after = pos + rinc;
        // the operation that holds row k * TP (the first row of tile k) opens the read's walk of that tile
        if (radv > 0 && first <= L - 1) {
            int lo = first > rd.row0 + 1 ? first : rd.row0 + 1;
            if (lo < 0) lo = 0;
            const int last_row = after - 1 < L - 1 ? after - 1 : L - 1;      // (an operation that ends before row 0 opens no tile)
            for (int k = (lo + TP - 1) / TP; k * TP <= last_row; ++k) put(tile0 + k, rd.c0 + i, first, ri + qinc - qadv);
        }
        pos += wave_total(rinc);
        if (FILL) ri += wave_total(qinc);
        if (pos > L - 1) break;
    }
}


// ---- packed form: clip + decode on the device -----------------------------------------------------------------------
// pa_bam_pack_regions (pepper_amd/csrc/bamio.cpp) ships every record as BAM stores it -- uint32 CIGAR words, 4-bit bases, one
// byte per quality -- once per batch; what the reference's get_reads does per (read, region) on the host (bam_handler.cpp:
// 176-303: walk the CIGAR, keep what lies inside [start, stop], decode the kept stretch of bases) is this kernel: one wave per
// (read, region) pair.  The walk has no running state here: 64 operations at a time, wave prefix sums give every operation its
// reference / read position, and what is kept of it follows from those plus one bit -- has an earlier operation kept an aligned
// base ("anchored": inserts, soft clips, deletions and skips are kept only behind one) [tests/bam_utils.py closed_form_clip is
// the same arithmetic in Python, checked against the sequential walk].  The kept bases are ONE stretch of the read
// (bamio.cpp, pa_bam_get_reads); it is decoded four bases per lane into the byte-per-base arrays tile_count_kernel reads.
struct PackedRead { int64_t data_off; int32_t pos, n_cigar, l_seq, flags; };     // = pa_packed_read
struct PairRec { int64_t s0; int32_t read, region, c0, cap; };                   // where the pair's clipped bases / operations go; cap > 0: room for that many bases only
static_assert(sizeof(PackedRead) == sizeof(pa_packed_read) && sizeof(PackedRead) == 24 && sizeof(PairRec) == 24, "packed tables");

struct UnpackArgs {
    const PairRec* pairs; int n_pairs;
    const PackedRead* preads; const RegRec* regions; const int64_t* region_start; const uint8_t* arena;
    const int64_t* seq_off;      // per packed read: where its bases and qualities lie when not behind its operations (-1), or null: none does
    ReadRec* reads; int32_t* cigar_op; int32_t* cigar_len; char* seq; uint8_t* qual;
    int* live;        // [n_regions] reads with a base inside | [n_regions] first inconsistent read + 1 | [n_regions + 1] first unsupported + 1
    int n_regions;
};

__global__ __launch_bounds__(256) void unpack_clip_kernel(UnpackArgs a) {
    const int pi = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pi >= a.n_pairs) return;
    const PairRec pr = a.pairs[pi];
    const PackedRead rd = a.preads[pr.read];
    const int64_t start = a.region_start[pr.region], stop = start + a.regions[pr.region].L - 1;
    typedef uint32_t __attribute__((aligned(1))) word_any;        // (a slice left in place in an inflated span sits at any byte)
    const word_any* cig = reinterpret_cast<const word_any*>(a.arena + rd.data_off);
    // positions relative to the region's start, clamped far outside it: a read that begins 2^30 bases in front of the region
    // would need operations the check below refuses anyway
    int64_t rel64 = (int64_t)rd.pos - start;
    int rpos = (int)(rel64 < -(1 << 30) ? -(1 << 30) : rel64);      // (rd.pos < stop: the packer's region test)
    const int last = (int)(stop - start);                            // rows 0 .. last are inside
    int ridx = 0, n_out = 0, written = 0, pos_start = 0, first_idx = 0;
    bool anchored = false, unsupported = false;
    for (int cb = 0; cb < rd.n_cigar; cb += 64) {
        const int i = cb + lane;
        const uint32_t c = i < rd.n_cigar ? cig[i] : 5u;             // (H: nothing)
        const int op = (int)(c & 15u), len = (int)(c >> 4);
        const bool isM = op == OP_M || op == OP_EQ || op == OP_X, isIS = op == OP_I || op == OP_S, isDN = op == OP_D || op == OP_N;
        if (__ballot(len >= (1 << 24))) { unsupported = true; break; }          // (prefix sums are 32-bit: 64 x 2^24 fits)
        const int radv = (isM || isDN) ? len : 0, qadv = (isM || isIS) ? len : 0;
        const int rinc = wave_inclusive_sum(radv), qinc = wave_inclusive_sum(qadv);
        const int rb = rpos + rinc - radv, qb = ridx + qinc - qadv;
        const int lo = rb > 0 ? rb : 0, hi = rb + len - 1 < last ? rb + len - 1 : last;
        const int kept_m = (isM && hi >= lo) ? hi - lo + 1 : 0;
        const unsigned long long mm = __ballot(kept_m > 0);
        const int first = mm ? __ffsll((long long)mm) - 1 : 64;
        const bool anch = anchored || lane > first;
        const bool inside = rb >= 0 && rb <= last;
        int kept = kept_m;
        if (isIS) kept = (inside && anch) ? len : 0;
        if (isDN) kept = (inside && anch) ? (len < last - rb + 1 ? len : last - rb + 1) : 0;
        if (!anchored && mm) {
            pos_start = __builtin_amdgcn_readlane(lo, first);
            first_idx = __builtin_amdgcn_readlane(qb + (rb < 0 ? -rb : 0), first);
            anchored = true;
        }
        const unsigned long long km = __ballot(kept > 0);
        if (kept > 0) {
            const int slot = pr.c0 + n_out + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(km >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)km, 0u));
            a.cigar_op[slot] = op;
            a.cigar_len[slot] = kept;
        }
        n_out += __popcll(km);
        written += wave_sum((isM || isIS) ? kept : 0);
        rpos += wave_total(rinc);
        ridx += wave_total(qinc);
        if (rpos > last) break;
    }
    if (pr.cap > 0 && written > pr.cap) unsupported = true;      // (the polish chain gives a pair the room a region can fill)
    const bool bad = !unsupported && written > 0 && ((unsigned)first_idx + (unsigned)written > (unsigned)rd.l_seq);
    if (lane == 0) {
        if (unsupported) atomicMax(&a.live[a.n_regions + 1], pr.read + 1);
        if (bad) atomicMax(&a.live[a.n_regions], pr.read + 1);
    }
    if (unsupported || bad) written = 0;
    if (lane == 0) {
        ReadRec out;
        out.s0 = pr.s0;
        out.c0 = pr.c0;
        out.ncig = written > 0 ? n_out : 0;
        out.slen = written;
        out.row0 = pos_start;
        out.region = pr.region;
        out.flags = ((rd.flags & 0x10) ? READ_REV : 0) | ((written > 0 && ((rd.flags >> 16) & 0xff) > 0) ? READ_MAPQ_OK : 0);
        a.reads[pi] = out;
        if (written > 0) atomicAdd(&a.live[pr.region], 1);
    }
    if (written <= 0) return;
    // the kept stretch: bases first_idx .. first_idx + written - 1 of the record, four per lane and step
    const int64_t apart = a.seq_off ? a.seq_off[pr.read] : -1;      // (a CIGAR kept in the CG tag: the bases stay in the record's core)
    const uint8_t* packed = a.arena + (apart >= 0 ? apart : rd.data_off + 4ll * rd.n_cigar);
    const uint8_t* quals = packed + (rd.l_seq + 1) / 2;
    const unsigned long long lut_lo = 0x565352474d43413dull;                // "=ACMGRSV", first letter in the low byte
    const unsigned long long lut_hi = 0x4e42444b48595754ull;                // "TWYHKDBN"
    uint32_t* seq_out = reinterpret_cast<uint32_t*>(a.seq + pr.s0);         // (s0 is a multiple of 4)
    uint32_t* qual_out = reinterpret_cast<uint32_t*>(a.qual + pr.s0);
    auto letter = [&](unsigned code) -> unsigned {
        const unsigned long long t = (code & 8u) ? lut_hi : lut_lo;
        return (unsigned)(t >> ((code & 7u) * 8u)) & 0xffu;
    };
    for (int j = lane; 4 * j < written; j += 64) {
        const int bidx = first_idx + 4 * j;
        const uint8_t* src = packed + (bidx >> 1);
        const unsigned p0 = src[0], p1 = src[1], p2 = src[2];               // (past the record's bases: its qualities / the arena's padding)
        unsigned c0, c1, c2, c3;
        if (bidx & 1) { c0 = p0 & 15u; c1 = p1 >> 4; c2 = p1 & 15u; c3 = p2 >> 4; }
        else { c0 = p0 >> 4; c1 = p0 & 15u; c2 = p1 >> 4; c3 = p1 & 15u; }
        seq_out[j] = letter(c0) | (letter(c1) << 8) | (letter(c2) << 16) | (letter(c3) << 24);
        const uint8_t* q = quals + bidx;
        qual_out[j] = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16) | ((unsigned)q[3] << 24);
    }
}

// ---- the reservoir sample of a deep interval (include/pepper_amd_encoder.h, pa_encoder_set_sampling) ------------------------
// The reference samples an interval's reads down to k = int(min(cap, rate * n)) with numpy.random.RandomState(seed) over the
// reads in read order (AlignmentSummarizer.py); n = the reads with a base inside, which only the clip kernel above knows.
// One workgroup per interval that can need it, between the clip and everything that reads the pairs: count the live pairs,
// run the sampler of reservoir.h (the generator's 624 words and the k <= 5000 slots in LDS; the whole workgroup regenerates
// and tempers the state -- three data-parallel stretches and the last word -- and ONE lane draws: n - k reads, 1 to 2 words
// each, in order; DESIGN.md 4.11 has what that costs), then clear every live pair whose rank is in no slot exactly as the
// clip kernel leaves a pair that keeps nothing.  The kept SET is what the later stages see (every count downstream is a sum
// over reads).
struct SampRec { int32_t region, pair0, pair1, pad; };
constexpr int RS_T = 256;            // threads of a workgroup: a stretch of the regeneration (227 words) fits one pass
constexpr int RS_CAP = 5000;         // slots in LDS: the largest max_reads pa_encoder_set_sampling takes
static_assert(PA_MT_S1 <= RS_T && PA_MT_S3 - PA_MT_S2 <= RS_T, "one regeneration stretch per pass of the workgroup");

__global__ __launch_bounds__(RS_T) void reservoir_keep_kernel(const SampRec* __restrict__ tab, ReadRec* __restrict__ reads,
                                                              int* __restrict__ live, uint8_t* __restrict__ keep,
                                                              int2* __restrict__ out, uint32_t seed, int cap, double rate) {
    __shared__ uint32_t mt[PA_MT_N], words[PA_MT_N];
    __shared__ int32_t slots[RS_CAP];
    __shared__ int wsum[RS_T / 64];
    __shared__ int s_n;
    __shared__ long long s_i;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const SampRec rec = tab[blockIdx.x];
    // n = the interval's reads: pairs that kept a base (ReadRec.slen = written > 0)
    if (tid == 0) s_n = 0;
    __syncthreads();
    int c = 0;
    for (int p = rec.pair0 + tid; p < rec.pair1; p += RS_T) c += reads[p].slen > 0 ? 1 : 0;
    c = wave_sum(c);
    if (lane == 0) atomicAdd(&s_n, c);
    __syncthreads();
    const int n = s_n;
    const int k = (int)pa_reservoir_allowed(cap, rate, n);      // (<= cap <= RS_CAP)
    if (tid == 0) out[blockIdx.x] = make_int2(n, n > k ? k : n);
    if (n <= k) return;                                          // nothing to do: the interval stays as the clip left it
    if (k > 0) {
        for (int i = tid; i < k; i += RS_T) slots[i] = i;
        if (tid == 0) {
            pa_mt_seed(mt, seed);
            s_i = k;
        }
        __syncthreads();
        for (;;) {
            for (int s = 0; s < 3; ++s) {
                const int lo = s == 0 ? 0 : (s == 1 ? PA_MT_S1 : PA_MT_S2), hi = s == 0 ? PA_MT_S1 : (s == 1 ? PA_MT_S2 : PA_MT_S3);
                const int kk = lo + tid;
                uint32_t word = 0;
                if (kk < hi) word = pa_mt_twist_word(mt[kk], mt[kk + 1], mt[pa_mt_far(kk)]);
                __syncthreads();                                 // (word kk + 1 is read before its owner replaces it)
                if (kk < hi) mt[kk] = word;
                __syncthreads();
            }
            if (tid == 0) mt[PA_MT_N - 1] = pa_mt_twist_word(mt[PA_MT_N - 1], mt[0], mt[PA_MT_M - 1]);
            __syncthreads();
            for (int p = tid; p < PA_MT_N; p += RS_T) words[p] = pa_mt_temper(mt[p]);
            __syncthreads();
            if (tid == 0) {
                int at = 0;
                s_i = pa_reservoir_draw(words, PA_MT_N, &at, s_i, n, k, slots);
            }
            __syncthreads();
            if (s_i >= n) break;
        }
    }
    // ranks in a slot, then the pairs in pair order again: a live pair whose rank is in none is cleared
    uint8_t* kp = keep + rec.pair0;
    for (int i = tid; i < n; i += RS_T) kp[i] = 0;
    __syncthreads();
    for (int i = tid; i < k; i += RS_T) kp[slots[i]] = 1;
    __syncthreads();
    int carry = 0;
    for (int base = rec.pair0; base < rec.pair1; base += RS_T) {
        const int p = base + tid;
        const int v = (p < rec.pair1 && reads[p].slen > 0) ? 1 : 0;
        const int inc = wave_inclusive_sum(v);
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int before = carry, total = 0;
        for (int q = 0; q < RS_T / 64; ++q) {
            if (q < w) before += wsum[q];
            total += wsum[q];
        }
        if (v && !kp[before + inc - 1]) {
            reads[p].ncig = 0;
            reads[p].slen = 0;
            reads[p].flags &= READ_REV;
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) live[rec.region] = k;
}

// ---- packed form: the read and pair tables built on the device ------------------------------------------------------------
// What pa_bam_pack_headers does on the host over the headers record_walk left in device memory (bamio.cpp: pack_walk's hdrs
// branch; the per-record rules are pack_rule.h, the same text): pack_scan_kernel -- ONE workgroup, the headers in file order
// PACK_BLOCK at a time with running carries, as tile_offsets_kernel scans -- finds the walk's end (a block minimum), the
// prefix maximum of the positions (which regions are closed), every kept record's run of regions (two binary searches) and
// its index in the read table (a prefix sum), writes the reads, snapshots what was complete when each region closed, adds up
// pairs / bases / operations per region, and leaves the summary; pack_fill_kernel -- one workgroup per closed region, the
// reads in file order PACK_BLOCK at a time -- gives the region's pairs their slots and their base / operation offsets.
// Spans hold thousands of records (2^18 at most): the order is what matters here, not the bandwidth.
constexpr int PACK_BLOCK = 1024;
struct PackHdr { int64_t data_off; int32_t ref_id, pos, l_seq, n_cigar, flags, ref_len, state, block_size; };    // = pa_record_header
static_assert(sizeof(PackHdr) == 40 && sizeof(pa_device_pack) == 64, "record header / pack summary");
enum { PK_CAP = 1, PK_CORRUPT = 2, PK_CG = 4, PK_OUTSIDE = 8, PK_WALK = 16 };          // what the scan met (bits)

struct PackArgs {
    const PackHdr* hdr;
    const int32_t* n_hdr_dev;        // the walk's record count and flags where the walk left them (null: n_hdr host entries uploaded)
    const int32_t* walk_flags_dev;
    int64_t n_hdr, hdr_cap;
    const int64_t* bounds_src; int64_t* bounds;      // start [n_regions] | stop [n_regions]: as handed over (mapped host memory or `bounds` itself), in device memory
    int32_t n_regions, tid, is_final, include_supplementary, min_mapq, split, reads_cap, pairs_cap;
    int64_t span_bytes;
    PackedRead* reads; int64_t* seq_off; int2* range;         // [reads_cap]: the table, the base offsets, each read's run of regions
    PairRec* pairs; int32_t* pair_read;                       // [pairs_cap]
    // [n_regions] each: pairs, bases, operations of a region; reads / slice bytes complete when it closed
    int32_t* r_pairs; unsigned long long* r_bases; unsigned long long* r_ops; int32_t* closed_reads; int64_t* closed_bytes;
    // the head: summary | region_pairs [n + 1] | op_base [n + 1] (pad to 8) | seq_base [n + 1] -- in device memory, and copied
    // into the page-locked block where that is mapped
    int32_t* head; int32_t* head_mapped; int32_t head_words;
};
__host__ __device__ inline size_t pack_head_ops(int n_regions) { return 64 + ((size_t)n_regions + 1) * 4; }
__host__ __device__ inline size_t pack_head_bases(int n_regions) { return (pack_head_ops(n_regions) + ((size_t)n_regions + 1) * 4 + 7) & ~(size_t)7; }
__host__ __device__ inline size_t pack_head_bytes(int n_regions) { return pack_head_bases(n_regions) + ((size_t)n_regions + 1) * 8; }

// inclusive scans over the wave for 64-bit sums and 32-bit maxima (lane shuffles; the 32-bit sums take wave_inclusive_sum)
__device__ __forceinline__ long long wave_inclusive_sum64(long long x) {
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const long long y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}
__device__ __forceinline__ int wave_inclusive_max(int x) {
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x = max(x, y);
    }
    return x;
}

__global__ __launch_bounds__(PACK_BLOCK) void pack_scan_kernel(PackArgs a) {
    __shared__ int w_min[16], w_max[16], w_cnt[16];
    __shared__ long long w_bytes[16];
    __shared__ int c_reads, c_max, c_met, c_split;
    __shared__ long long c_bytes;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nreg = a.n_regions;
    int64_t n = a.n_hdr;
    int met0 = 0;
    if (a.n_hdr_dev) {
        n = *a.n_hdr_dev;
        if (n < 0 || n > a.hdr_cap || a.walk_flags_dev[0] != 0) { n = 0; met0 = PK_WALK; }
    }
    if (tid == 0) { c_reads = 0; c_max = INT_MIN; c_met = met0; c_split = 0; c_bytes = 0; }
    if (a.bounds_src != a.bounds)                // (one trip over the bus instead of one per step of every binary search)
        for (int k = tid; k < 2 * nreg; k += PACK_BLOCK) a.bounds[k] = a.bounds_src[k];
    const int64_t* r_start = a.bounds;
    const int64_t* r_stop = a.bounds + nreg;
    for (int r = tid; r < nreg; r += PACK_BLOCK) {
        a.r_pairs[r] = 0; a.r_bases[r] = 0; a.r_ops[r] = 0; a.closed_reads[r] = 0; a.closed_bytes[r] = 0;
    }
    __threadfence();
    __syncthreads();
    const int64_t last_stop = r_stop[nreg - 1];
    bool ended = false;
    for (int64_t base = 0; base < n && !ended; base += PACK_BLOCK) {
        const int64_t i = base + tid;
        PackHdr h{};
        int cls = pa_pack::HDR_SKIP;
        if (i < n) {
            h = a.hdr[i];
            cls = pa_pack::header_class(h.ref_id, h.pos, a.tid, last_stop);
        }
        // the first header of the block that ends the walk (a corrupt one ends it with an error)
        const bool corrupt = i < n && h.state == 2;
        const int wm = wave_min((cls == pa_pack::HDR_STOP || corrupt) ? tid : PACK_BLOCK);
        if (lane == 0) w_min[w] = wm;
        __syncthreads();
        int first = PACK_BLOCK;
        for (int k = 0; k < 16; ++k) first = min(first, w_min[k]);
        ended = first < PACK_BLOCK;
        if (tid == first && corrupt) atomicOr(&c_met, PK_CORRUPT);
        const bool active = i < n && tid < first && cls == pa_pack::HDR_CONTIG;
        // the furthest position seen up to each header: the regions whose stop it has reached are closed
        const int pinc = wave_inclusive_max(active ? h.pos : INT_MIN);
        if (lane == 63) w_max[w] = pinc;
        __syncthreads();
        int pm_before = c_max;
        for (int k = 0; k < w; ++k) pm_before = max(pm_before, w_max[k]);
        int p_prev = __shfl_up(pinc, 1, 64);
        if (lane == 0) p_prev = INT_MIN;
        const int pm_excl = max(pm_before, p_prev);
        const int pm_incl = max(pm_before, pinc);
        int lo = 0, hi = 0;
        bool is_read = false;
        int64_t bytes = 0, seq_at = -1;
        if (active) {
            lo = pa_pack::first_open_region(r_stop, nreg, pm_incl);
            const uint32_t flag = (uint32_t)h.flags & 0xffffu;
            const int mapq = (h.flags >> 16) & 0xff;
            hi = lo;
            if (!pa_pack::record_dropped(flag, mapq, (uint32_t)h.l_seq, (uint32_t)h.n_cigar, a.include_supplementary, a.min_mapq))
                hi = pa_pack::region_range_end(r_start, nreg, lo, pa_pack::read_end(h.pos, h.ref_len));
            is_read = hi > lo;
        }
        if (is_read) {
            int met = 0;
            if (h.state == 1 || (h.state == 3 && !a.split)) met |= PK_CG;
            if (h.state == 3) {
                seq_at = h.data_off - (int64_t)h.block_size;
                if (h.block_size <= 0 || seq_at < 0) met |= PK_OUTSIDE;
            }
            // the arena test of the host's staging: both slices inside the resident span, before anything dereferences them
            if (h.n_cigar < 0 || h.l_seq < 0 || h.data_off < 0) {
                met |= PK_OUTSIDE;
            } else {
                const int64_t ops_end = h.data_off + 4ll * h.n_cigar, bases = ((int64_t)h.l_seq + 1) / 2 + h.l_seq;
                if (seq_at < 0 ? ops_end + bases > a.span_bytes : (ops_end > a.span_bytes || seq_at + bases > a.span_bytes)) met |= PK_OUTSIDE;
            }
            if (met) atomicOr(&c_met, met);
            bytes = pa_pack::slice_bytes((uint32_t)h.n_cigar, (uint32_t)h.l_seq);
        }
        const int rinc = wave_inclusive_sum(is_read ? 1 : 0);
        const long long binc = wave_inclusive_sum64(bytes);
        if (lane == 63) { w_cnt[w] = rinc; w_bytes[w] = binc; }
        __syncthreads();
        int r_before = c_reads;
        long long b_before = c_bytes;
        for (int k = 0; k < w; ++k) { r_before += w_cnt[k]; b_before += w_bytes[k]; }
        const int ri = r_before + rinc - (is_read ? 1 : 0);
        const long long b_excl = b_before + binc - bytes;
        if (active) {
            // what was complete when this header closed its regions: the reads and bytes in front of it
            const int lo_prev = pa_pack::first_open_region(r_stop, nreg, pm_excl);
            for (int k = lo_prev; k < lo; ++k) { a.closed_reads[k] = ri; a.closed_bytes[k] = b_excl; }
        }
        if (is_read && ri < a.reads_cap) {
            a.reads[ri] = PackedRead{h.data_off, h.pos, h.n_cigar, h.l_seq, (int32_t)((uint32_t)h.flags & 0x00ffffffu)};
            a.seq_off[ri] = seq_at;
            a.range[ri] = make_int2(lo, hi);
            const unsigned long long room = (unsigned long long)pa_pack::base_room(h.l_seq);
            for (int r = lo; r < hi; ++r) {
                atomicAdd(&a.r_pairs[r], 1);
                atomicAdd(&a.r_bases[r], room);
                atomicAdd(&a.r_ops[r], (unsigned long long)(uint32_t)h.n_cigar);
            }
        }
        __syncthreads();
        if (tid == PACK_BLOCK - 1) { c_reads = r_before + rinc; c_bytes = b_before + binc; c_max = pm_incl; }
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    // the summary (one lane: a few dozen regions)
    pa_device_pack* sum = reinterpret_cast<pa_device_pack*>(a.head);
    int32_t* region_pairs = a.head + 16;
    int32_t* op_base = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(a.head) + pack_head_ops(nreg));
    int64_t* seq_base = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(a.head) + pack_head_bases(nreg));
    if (tid == 0) {
        int met = c_met;
        const bool cut = !ended && !a.is_final;
        const int n_closed = cut ? pa_pack::first_open_region(r_stop, nreg, c_max) : nreg;
        const int total_reads = c_reads;
        if (total_reads > a.reads_cap) met |= PK_CAP;
        long long all_pairs = 0, pairs = 0, bases = 0, ops = 0;
        region_pairs[0] = 0; op_base[0] = 0; seq_base[0] = 0;
        for (int r = 0; r < nreg; ++r) {
            const long long np = __hip_atomic_load(&a.r_pairs[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            all_pairs += np;
            if (r < n_closed) {
                const long long rb = (long long)__hip_atomic_load(&a.r_bases[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                pairs += np;
                bases += rb;
                ops += (long long)__hip_atomic_load(&a.r_ops[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (rb > 0xffffff00ll || ops > 0x7ffffff0ll) met |= PK_OUTSIDE;        // (the staging's limits: 2^32 bases per region, 2^31 operations)
            }
            region_pairs[r + 1] = (int32_t)(pairs < 0x7fffffff ? pairs : 0x7fffffff);
            op_base[r + 1] = (int32_t)(ops < 0x7fffffff ? ops : 0x7fffffff);
            seq_base[r + 1] = bases;
        }
        if (all_pairs > a.pairs_cap) met |= PK_CAP;
        int status = 0;
        if (met & PK_WALK) status = 6;
        else if (met & PK_CORRUPT) status = 2;
        else if (met & PK_CG) status = 3;
        else if (met & PK_CAP) status = 1;
        else if (cut && n_closed == 0) status = 4;
        else if (met & PK_OUTSIDE) status = 5;
        sum->status = status;
        sum->n_done = status ? 0 : n_closed;
        sum->n_reads = status ? 0 : ((cut && n_closed > 0) ? a.closed_reads[n_closed - 1] : total_reads);
        sum->n_pairs = status ? 0 : (int32_t)pairs;
        sum->n_split = 0;
        sum->walk_flags[0] = a.walk_flags_dev ? a.walk_flags_dev[0] : 0;
        sum->walk_flags[1] = a.walk_flags_dev ? a.walk_flags_dev[1] : 0;
        sum->reserved = 0;
        sum->n_headers = n;
        sum->slice_bytes = status ? 0 : ((cut && n_closed > 0) ? a.closed_bytes[n_closed - 1] : c_bytes);
        sum->total_bases = status ? 0 : bases;
        sum->total_ops = status ? 0 : ops;
    }
    __threadfence();
    __syncthreads();
    // reads of the kept table whose bases lie apart from their operations
    {
        const int kept = sum->n_reads;
        int mine = 0;
        for (int k = tid; k < kept; k += PACK_BLOCK) mine += a.seq_off[k] >= 0 ? 1 : 0;
        mine = wave_sum(mine);
        if (lane == 0 && mine) atomicAdd(&c_split, mine);
        __syncthreads();
        if (tid == 0) sum->n_split = c_split;
        __threadfence();
        __syncthreads();
    }
    if (a.head_mapped)
        for (int k = tid; k < a.head_words; k += PACK_BLOCK) a.head_mapped[k] = a.head[k];
}

// one workgroup per closed region: its reads in file order, each pair's slot and where its clipped bases / operations go
// (the running sums of the host's staging: pa_pack::base_room(l_seq) bases and n_cigar operations per pair)
__global__ __launch_bounds__(PACK_BLOCK) void pack_fill_kernel(PackArgs a) {
    __shared__ int w_cnt[16], w_ops[16];
    __shared__ long long w_bases[16];
    __shared__ int c_cnt, c_ops;
    __shared__ long long c_bases;
    const pa_device_pack* sum = reinterpret_cast<const pa_device_pack*>(a.head);
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (sum->status != 0 || r >= sum->n_done) return;
    const int nreg = a.n_regions, n_reads = min(sum->n_reads, a.reads_cap);
    const int32_t* region_pairs = a.head + 16;
    const int slot0 = region_pairs[r], slot1 = region_pairs[r + 1];
    const int ops0 = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(a.head) + pack_head_ops(nreg))[r];
    const long long bases0 = reinterpret_cast<const int64_t*>(reinterpret_cast<const char*>(a.head) + pack_head_bases(nreg))[r];
    if (tid == 0) { c_cnt = 0; c_ops = 0; c_bases = 0; }
    __syncthreads();
    for (int base = 0; base < n_reads; base += PACK_BLOCK) {
        const int ri = base + tid;
        bool in = false;
        int ops = 0;
        long long room = 0;
        if (ri < n_reads) {
            const int2 rg = a.range[ri];
            in = rg.x <= r && r < rg.y;
            if (in) {
                const PackedRead rd = a.reads[ri];
                ops = rd.n_cigar;
                room = pa_pack::base_room(rd.l_seq);
            }
        }
        const int cinc = wave_inclusive_sum(in ? 1 : 0), oinc = wave_inclusive_sum(ops);
        const long long binc = wave_inclusive_sum64(room);
        if (lane == 63) { w_cnt[w] = cinc; w_ops[w] = oinc; w_bases[w] = binc; }
        __syncthreads();
        int c_before = c_cnt, o_before = c_ops;
        long long b_before = c_bases;
        for (int k = 0; k < w; ++k) { c_before += w_cnt[k]; o_before += w_ops[k]; b_before += w_bases[k]; }
        const int slot = slot0 + c_before + cinc - 1;
        if (in && slot < slot1 && slot < a.pairs_cap) {
            a.pair_read[slot] = ri;
            a.pairs[slot] = PairRec{bases0 + b_before + binc - room, ri, r, ops0 + o_before + oinc - ops, 0};
        }
        __syncthreads();
        if (tid == PACK_BLOCK - 1) { c_cnt = c_before + cinc; c_ops = o_before + oinc; c_bases = b_before + binc; }
        __syncthreads();
    }
}

// exclusive scan of the per-tile record counts (one workgroup; tiles per batch: 12.5 k for 64 regions of 100 kb)
__global__ __launch_bounds__(1024) void tile_offsets_kernel(const int* __restrict__ tile_count, int n_tiles, int* __restrict__ tile_off) {
    __shared__ int wsum[16];
    __shared__ int carry;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n_tiles; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < n_tiles ? tile_count[i] : 0;
        const int inc = wave_inclusive_sum(v);
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int before = carry;
        for (int k = 0; k < w; ++k) before += wsum[k];
        if (i < n_tiles) tile_off[i] = before + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = before + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_off[n_tiles] = carry;
}

// ---- targets (pa_encoder_set_targets) --------------------------------------------------------------------------------
// One verdict per matrix row of the batch, laid out like `pass`: is the row's contig position inside one of the n disjoint,
// ascending half-open intervals [t_start[i], t_end[i])?  One workgroup per tile, four rows per thread (row_base is a multiple
// of 16 and a tile starts at a multiple of 512: every thread stores one aligned word).  The workgroup's stretch of the table
// -- the intervals that can touch its 512 positions -- comes from two binary searches whose every operand is the same in all
// lanes; a thread then searches that stretch (at most 257 intervals) for its first row and steps through its other three.
constexpr int TRT = TP / 4;
__global__ __launch_bounds__(TRT) void target_rows_kernel(const RegRec* __restrict__ regions, const int32_t* __restrict__ tile_region,
                                                          const int64_t* __restrict__ t_start, const int64_t* __restrict__ t_end,
                                                          int64_t n, uint8_t* __restrict__ targets) {
    const int tile = blockIdx.x;
    const RegRec* reg = regions + tile_region[tile];
    const int tile_lo = (tile - reg->tile0) * TP;
    const int rows = (reg->L + 1 + 15) & ~15;      // the rows of `targets` that are this region's (region_pass)
    const int64_t p0 = reg->region_start + tile_lo;
    int64_t lo = 0, hi = n;                        // first interval that ends behind the tile's first position
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (t_end[mid] > p0) hi = mid; else lo = mid + 1;
    }
    const int64_t first = lo;
    hi = n;                                        // first interval that starts behind the tile's last position
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (t_start[mid] >= p0 + TP) hi = mid; else lo = mid + 1;
    }
    const int64_t last = lo;
    const int r0 = tile_lo + 4 * (int)threadIdx.x;
    if (r0 >= rows) return;
    const int64_t p = reg->region_start + r0;
    int64_t k = first;                             // first interval of the stretch that ends behind p
    hi = last;
    while (k < hi) {
        const int64_t mid = k + ((hi - k) >> 1);
        if (t_end[mid] > p) hi = mid; else k = mid + 1;
    }
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        while (k < last && t_end[k] <= p + j) ++k;
        if (k < last && t_start[k] <= p + j) word |= 1u << (8 * j);
    }
    *reinterpret_cast<uint32_t*>(targets + reg->row_base + r0) = word;
}

// ---- the tile kernel -----------------------------------------------------------------------------------------------
struct TileArgs {
    const ReadRec* reads; const RegRec* regions; const int32_t* tile_region;
    const int32_t* cigar_op; const int32_t* cigar_len; const char* seq; const uint8_t* qual; const char* ref;
    const TileRec* recs; const int* tile_off; int rec_cap;
    int* mat; uint8_t* pass; SiteRec* sites; Vote* votes; Vote* votes_out; int vote_cap; int4* ovf; int ovf_cap; int* counters;
    int* region_counts;
    const uint8_t* targets;   // verdicts of target_rows_kernel, one per row like `pass`; null: no targets set
    int32_t* depth;           // tile_count_kernel<true>: the row's coverage as the per-position pass sees it, one int32 per row like `pass`
    int debug;        // PA_TILE_DEBUG (profiling only, tools/tile_ablation.sh): parts of the kernel switched off
    uint8_t* gq;              // tile_count_kernel<TILE_REFCONF>: the row's reference-confidence GQ, one byte per row like `pass` ...
    const uint8_t* gq_table;  // ... looked up in the host's REFCONF_SIDE x REFCONF_SIDE table [n_ref][n_alt] (pa_encoder_set_ref_confidence)
};

__device__ __forceinline__ uint64_t allele_prefix(const char* bytes, uint32_t off, uint32_t len) {
    uint64_t p = 0;
    for (uint32_t k = 0; k < 8; ++k) p = (p << 8) | (k < len ? (uint64_t)(unsigned char)bytes[(size_t)off + k] : 0);
    return p;
}

// Append v to the global list `out` (counter `count`) from the lanes where `has`: one global atomic per wave.
__device__ __forceinline__ void wave_append_vote(bool has, const Vote& v, Vote* out, int* count, int cap, int lane) {
    const unsigned long long m = __ballot(has);
    if (!m) return;
    int base = 0;
    const int leader = __ffsll((long long)m) - 1;
    if (lane == leader) base = atomicAdd(count, __popcll(m));
    base = __builtin_amdgcn_readlane(base, leader);
    const int slot = base + __popcll(m & ((1ull << lane) - 1ull));
    if (has && slot < cap) out[slot] = v;
}

#ifndef PA_TILE_MIN_WAVES
#define PA_TILE_MIN_WAVES 4          // measured equal at 4 / 6 / 8 (2 / 3 / 4 workgroups per CU); 6 and 8 spill 7 / 19 registers to scratch
#endif
#ifdef PA_ENC_STAMP
__device__ unsigned long long g_enc_cycles[8];     // debug: shader-clock cycles per phase, summed over the waves
#define ENC_LAP(k) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); lap_acc[k] += t_ - lap_t; lap_t = t_; } while (0)
#else
#define ENC_LAP(k) do { } while (0)
#endif
// FORM: what the per-position pass keeps beside the matrix row.  TILE_PLAIN nothing; TILE_DEPTH (depth bins set,
// pa_encoder_set_depth_bins) the row's coverage; TILE_REFCONF (a reference-confidence table set, pa_encoder_set_ref_confidence,
// with or without depth bins) the coverage and the row's GQ byte: the evidence of variant/RefConfidence.py from the counters
// before the int8 clamp, rescaled to 100 and looked up -- no transcendental runs here.  A template parameter and not a test of
// a.depth / a.gq: the instance every other run launches is then instruction for instruction the kernel without the feature
// (with the test in it the register allocation moved and the kernel measured 6 % slower, switch off).
enum { TILE_PLAIN = 0, TILE_DEPTH = 1, TILE_REFCONF = 2 };
constexpr int REFCONF_SIDE = 101;                  // the table's side: counts 0 .. 100 after the rescale
template <int FORM>
__global__ __launch_bounds__(NT, PA_TILE_MIN_WAVES) void tile_count_kernel(TileArgs a) {
    __shared__ int cnt[NCNT * TP];                 // [counter][row]; reused as the finished [row][26] tile for the store
    __shared__ char ref_s[TP];
    __shared__ uint8_t refok_s[TP];               // is_acgt(reference base) per row
    __shared__ int4 s_ent[NW][64];                 // per wave: the reference-consuming operations of the batch that touch the span, in order
    __shared__ unsigned s_mask[NW][16];            // per wave: bit k = an operation's share of the span starts at row span_lo + k
    __shared__ uint2 vbuf[VCAP];                   // indel allele votes of this tile: only those of passing rows leave the CU
    __shared__ int vcount;
    // A base of a match run that equals an A/C/G/T reference base and passes the quality test -- 95 % of all bases -- adds one
    // to the coverage, to its strand's coverage (unless it anchors an insert / a deletion) and to its strand's column of that
    // letter.  Those three go in per RUN, as +1 / -1 at the run's ends in a difference array (two LDS atomics per operation
    // instead of three per base; the prefix sums are taken once, when the tile is complete); the row phase only looks at each
    // base (quality, letter, reference letter) and queues the ones that are NOT of that kind, which are then processed 64 at
    // a time with the full rules plus the undoing of what the run assumed for them.
    __shared__ int mcov[2][TP + 8];                // [strand][row]: match runs starting minus match runs ended before this row
    __shared__ int anch[TP];                       // runs whose last base sits here and anchors an insert / a deletion: forward | reverse << 16
    __shared__ unsigned xq[NW][XQ];                // queued bases: row | letter << 9 | quality ok << 17 | anchoring << 18 | reverse << 19
    __shared__ int wtot[2][NW];
    __shared__ int s_out[4];                       // passing sites / votes of the tile; their first slots in the region's lists
    uint8_t* pass_s = reinterpret_cast<uint8_t*>(&xq[0][0]);   // verdicts of the per-position pass: the queues are empty by then (two
                                                               // workgroups per CU need the tile's LDS below 80 KB)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int tile = blockIdx.x;
    const int region = a.tile_region[tile];
    const RegRec reg = a.regions[region];
    const int L = reg.L;
    const int tile_lo = (tile - reg.tile0) * TP, tile_hi = tile_lo + TP - 1;
    const int live_max = tile_hi + 1 < L - 1 ? tile_hi + 1 : L - 1;   // operations starting past this row are not this tile's (pos > end: not walked at all)
    for (int i = tid; i < NCNT * TP; i += NT) cnt[i] = 0;
    for (int i = tid; i < 2 * (TP + 8); i += NT) (&mcov[0][0])[i] = 0;
    if (tid < TP) anch[tid] = 0;
    if (tid < TP) {
        const int idx = tile_lo + tid;
        ref_s[tid] = idx < reg.ref_len ? a.ref[reg.ref_off + idx] : 'N';
        refok_s[tid] = is_acgt(ref_s[tid]) ? 1 : 0;
    }
    if (tid == 0) vcount = 0;
    if (tid < 4) s_out[tid] = 0;
    __syncthreads();

    const int rec0 = a.tile_off[tile], rec1 = (a.debug & 1) ? rec0 : (a.tile_off[tile + 1] < a.rec_cap ? a.tile_off[tile + 1] : a.rec_cap);
    int4* ent_s = s_ent[w];
    unsigned* mask_s = s_mask[w];
    // the wave's queue of bases that need the full rules: `qn` entries (wave-uniform), drained 64 at a time
    unsigned* xq_w = xq[w];
    int qn = 0;
    auto drain = [&](int count) {                  // entries [0, count) of the queue, one per lane
        const bool on = lane < count;
        const unsigned e = on ? xq_w[lane] : 0u;
        const int o = (int)(e & 511u);
        const unsigned b = (e >> 9) & 255u;
        const bool q_ok = on && ((e >> 17) & 1u), anchoring = (e >> 18) & 1u, erev = (e >> 19) & 1u;
        const unsigned rb = (unsigned char)ref_s[o];
        const unsigned ru = rb & 0xDFu, bu = b & 0xDFu;
        const unsigned ridx = (ru >> 1) & 3u, bidx = (bu >> 1) & 3u;
        const bool ref_ok = ((0x47544341u >> (ridx * 8)) & 0xFFu) == ru;            // is_acgt(reference base)
        const unsigned letter = (0x47544341u >> (bidx * 8)) & 0xFFu;
        const int acgt = (int)(bidx ^ (bidx >> 1));                                  // A C G T -> 0 1 2 3
        const int racgt = (int)(ridx ^ (ridx >> 1));
        const int sym = letter == bu ? acgt : (bu == 'I' ? 4 : (bu == 'D' ? 5 : 6));   // symbol_column's switch
        const bool mism = q_ok && rb != b;                                           // case-sensitive, as the reference compares
        const bool plain = letter == b;                                              // an upper-case A C G T: tallied on the device
        const int strand = erev ? K_REV : K_FWD;
        // what the rules give this base (:357-430) minus what its run assumed for it (coverage, strand coverage unless
        // anchoring, the reference letter's column where the reference base is a letter)
        atomicAdd(&cnt[K_COV * TP + o], on ? (q_ok ? 0 : -1) : 0);
        atomicAdd(&cnt[strand * TP + o], (on && !anchoring && !q_ok) ? -1 : 0);
        atomicAdd(&cnt[(strand + 1 + racgt) * TP + o], (on && ref_ok) ? -1 : 0);
        atomicAdd(&cnt[(strand + 1 + sym) * TP + o], (q_ok && ref_ok) ? 1 : 0);
        atomicAdd(&cnt[K_SNP * TP + o], mism ? 1 : 0);
        atomicAdd(&cnt[(K_TAB + (erev ? 4 : 0) + acgt) * TP + o], (mism && plain) ? 1 : 0);
        if (mism && !plain) {                        // rare alphabet (N, IUPAC, lower case): exact key kept on host
            const int slot = atomicAdd(&a.counters[CT_OVF], 1);
            if (slot < a.ovf_cap) a.ovf[slot] = make_int4(o + tile_lo, (int)b, erev ? 1 : 0, region);
        }
    };
    TileRec rec{0, 0, 0, 0};
    if (rec0 + w < rec1) rec = a.recs[rec0 + w];
    for (int k = rec0 + w; k < rec1; k += NW) {
        // three independent loads: the read's table entry, the first 64 operations (the arrays are padded: no bound needed
        // to issue them), and the next record of this wave
        const ReadRec rd_v = a.reads[rec.read];
        int op_ld = a.cigar_op[rec.op + lane], len_ld = a.cigar_len[rec.op + lane], next_ld = a.cigar_op[rec.op + lane + 1];
        TileRec rec_next = rec;
        if (k + NW < rec1) rec_next = a.recs[k + NW];
        // the record and the read's entry are the same in every lane: keep them in scalar registers
        struct { int64_t s0; int32_t c0, ncig, slen, flags; } rd;
        rd.s0 = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(rd_v.s0 >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_readfirstlane((int)rd_v.s0));
        rd.c0 = __builtin_amdgcn_readfirstlane(rd_v.c0);
        rd.ncig = __builtin_amdgcn_readfirstlane(rd_v.ncig);
        rd.slen = __builtin_amdgcn_readfirstlane(rd_v.slen);
        rd.flags = __builtin_amdgcn_readfirstlane(rd_v.flags);
        rec.read = __builtin_amdgcn_readfirstlane(rec.read);
        rec.op = __builtin_amdgcn_readfirstlane(rec.op);
        rec.row = __builtin_amdgcn_readfirstlane(rec.row);
        rec.ri = __builtin_amdgcn_readfirstlane(rec.ri);
        const uint8_t* qual0 = a.qual + rd.s0;         // scalar base + 32-bit lane offset
        const char* seq0 = a.seq + rd.s0;
        const bool rev = rd.flags & READ_REV;
        const int c_end = rd.c0 + rd.ncig;
        int pos = rec.row, ri = rec.ri;
        ENC_LAP(0);                                   // record set-up (waits for the prefetched loads)
        for (int c = rec.op; c < c_end; c += 64) {
            const int i = c + lane;
            if (c != rec.op) {
                op_ld = a.cigar_op[i];
                len_ld = a.cigar_len[i];
                next_ld = a.cigar_op[i + 1];
            }
            const bool valid = i < c_end;
            const int op = valid ? op_ld : OP_H;
            const int len = valid ? len_ld : 0;
            const int next_op = i + 1 < c_end ? next_ld : -1;
            const int radv = variant_ref_advance(op, len), qadv = variant_read_advance(op, len);
            const int rinc = wave_inclusive_sum(radv), qinc = wave_inclusive_sum(qadv);
            const int first = pos + rinc - radv, rfirst = ri + qinc - qadv;
            const int total_r = wave_total(rinc);
            const bool live = valid && first <= live_max;
            const int anchor = first - 1;                                   // row an insert / a deletion is credited to
            const bool mine = live && anchor >= tile_lo && anchor <= tile_hi;   // (anchor <= L - 2 follows from first <= L - 1)
            const bool is_ins = mine && op == OP_I && rfirst - 1 >= 0 && !(a.debug & 8);
            const int n_ins = len + 1;
            const int span_lo = pos > tile_lo ? pos : tile_lo;
            int span_hi = pos + total_r - 1;
            if (span_hi > tile_hi) span_hi = tile_hi;
            if (span_hi > L - 1) span_hi = L - 1;

            // -- an insert's qualities (its anchor base and its first seven bases: nearly every insert is that short) as two
            //    unaligned dwords, asked for FIRST: they are back before the row phase's sixteen byte loads, which are asked for
            //    next and which the per-operation section would otherwise wait behind (loads return in order)
            typedef unsigned __attribute__((aligned(1))) u32u;
            const unsigned q_at = is_ins ? (unsigned)(rfirst - 1) : 0u;
            const unsigned qw0 = *reinterpret_cast<const u32u*>(qual0 + q_at), qw1 = *reinterpret_cast<const u32u*>(qual0 + q_at + 4);
            // -- scratch for the row phase.  Every row of the span belongs to the reference-consuming operation that covers it:
            //    those operations are compacted, in order, into {first row, read index there, last row, code | anchoring bit}
            //    entries, and each marks the row where its share of the span starts in a 512-bit mask.  A row's owner is then
            //    the number of marks at or before it (one broadcast read of the mask + mbcnt) instead of a six-step binary
            //    search over the first rows -- the kernel is bound by what it asks of the LDS (16 wave-instructions per 64 rows
            //    before this, each a round trip that four waves per SIMD have little to cover with).
            const int last = first + radv - 1;
            const bool cons = valid && radv > 0 && last >= span_lo && first <= span_hi;
            const unsigned long long cm = __ballot(cons);
            if (lane < 16) mask_s[lane] = 0u;
            __builtin_amdgcn_wave_barrier();
            if (cons) {
                const int cidx = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(cm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)cm, 0u));
                // bit 4: an insert or a deletion follows, so the last base of this match run anchors it (:381-391)
                ent_s[cidx] = make_int4(first, rfirst, last, op | ((next_op == OP_I || next_op == OP_D) ? 16 : 0));
                const int kk = (first > span_lo ? first : span_lo) - span_lo;
                atomicOr(&mask_s[kk >> 5], 1u << (kk & 31));
            }
            __builtin_amdgcn_wave_barrier();

            // -- one match run per lane: its clipped ends into the difference array of its strand, its anchoring last base
            {
                const bool match_op = valid && (op == OP_M || op == OP_EQ || op == OP_X) && len > 0;
                const int lo = first > span_lo ? first : span_lo;
                const int hi = last < span_hi ? last : span_hi;
                if (match_op && lo <= hi && !(a.debug & 64)) {
                    atomicAdd(&mcov[rev ? 1 : 0][lo - tile_lo], 1);
                    atomicAdd(&mcov[rev ? 1 : 0][hi + 1 - tile_lo], -1);
                    if ((next_op == OP_I || next_op == OP_D) && hi == last) atomicAdd(&anch[hi - tile_lo], rev ? 0x10000 : 1);
                }
            }

            // -- the row phase's loads first: one reference row per lane, UNR rows in flight; owners by binary search over the
            //    scratch, then every quality / base byte load of the (read, tile) is issued before anything waits on one
            bool is_m[UNR], is_d[UNR], anchored[UNR];
            int pl[UNR], qv[UNR];
            char bv[UNR];
            bool past = false;
            {
                unsigned si[UNR];
                int before = 0;                           // marks in the blocks in front of this one (wave-uniform)
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int p = span_lo + lane + 64 * u;
                    const bool act = p <= span_hi;
                    // a lane past the span keeps a row of its own (its add is a zero): equal addresses would serialise in the LDS
                    const int pc = act ? p : tile_lo + ((lane + 64 * u) & (TP - 1));
                    const unsigned m_lo = __builtin_amdgcn_readfirstlane(mask_s[2 * u]), m_hi = __builtin_amdgcn_readfirstlane(mask_s[2 * u + 1]);
                    const unsigned own = ((lane < 32 ? m_lo >> lane : m_hi >> (lane - 32)) & 1u);
                    int j = before + (int)__builtin_amdgcn_mbcnt_hi(m_hi, __builtin_amdgcn_mbcnt_lo(m_lo, 0u)) + (int)own - 1;
                    before += __popc(m_lo) + __popc(m_hi);
                    j = (act && j > 0) ? j : 0;
                    const int4 e = ent_s[j];
                    const int oj = e.w & 15;
                    const int rp = e.y + (pc - e.x);
                    const bool m = act && (oj == OP_M || oj == OP_EQ || oj == OP_X);
                    const bool inb = (unsigned)rp < (unsigned)rd.slen;
                    past |= m && !inb;
                    is_m[u] = m && inb;
                    is_d[u] = act && oj == OP_D;
                    anchored[u] = (e.w & 16) && pc == e.z;
                    pl[u] = pc - tile_lo;
                    si[u] = is_m[u] ? (unsigned)rp : 0u;       // (a lane without a base loads the read's first byte: no exec mask)
                }
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    qv[u] = (int)__builtin_nontemporal_load(qual0 + si[u]);
                    bv[u] = __builtin_nontemporal_load(seq0 + si[u]);
                }
            }
            if (past) atomicMax(&a.counters[CT_ERR], rec.read + 1);    // CIGAR runs past the sequence: reported by the host
            ENC_LAP(1);                               // scans, scratch, owner search, byte loads issued

            // -- one operation per lane: inserts (:431-490) and deletion anchors (:491-540)
            long long qsum = 0;
            if (is_ins) {
                // bytes 0 .. min(n_ins, bases left in the read, 8) - 1 of the two dwords
                int take = n_ins < rd.slen - (rfirst - 1) ? n_ins : rd.slen - (rfirst - 1);
                take = take < 8 ? (take > 0 ? take : 0) : 8;
                const unsigned m0 = take >= 4 ? 0xffffffffu : ((1u << (8 * take)) - 1u);
                const unsigned m1 = take >= 8 ? 0xffffffffu : (take > 4 ? ((1u << (8 * (take - 4))) - 1u) : 0u);
                qsum = (long long)__builtin_amdgcn_sad_u8(qw0 & m0, 0u, __builtin_amdgcn_sad_u8(qw1 & m1, 0u, 0u));
                if (n_ins <= 33)
                    for (int q = 8; q < n_ins; ++q) qsum += rfirst - 1 + q < rd.slen ? qual0[(unsigned)(rfirst - 1 + q)] : 0;
            }
            for (unsigned long long big = __ballot(is_ins && n_ins > 33); big; big &= big - 1) {   // long inserts: the wave sums
                const int src = __ffsll((long long)big) - 1;
                const int n = __builtin_amdgcn_readlane(n_ins, src), r0 = __builtin_amdgcn_readlane(rfirst, src) - 1;
                int part = 0;
                for (int q = lane; q < n; q += 64) part += r0 + q < rd.slen ? qual0[(unsigned)(r0 + q)] : 0;
                const int total = wave_sum(part);
                if (lane == src) qsum = total;
            }
            bool vote = false;
            unsigned vmeta = 0, voff = 0;
            if (is_ins) {
                const int avail = n_ins < rd.slen - (rfirst - 1) ? n_ins : (rd.slen - (rfirst - 1) > 0 ? rd.slen - (rfirst - 1) : 0);
                const bool passes = (double)qsum >= reg.min_indel_q * (double)n_ins;
                const int al = anchor - tile_lo;
                // (the reference reads the anchor base's quality without a bound; a CIGAR that ends past the sequence is an error here)
                const int anchor_q = rfirst - 1 < rd.slen ? (int)(qw0 & 255u) : 0;
                if (passes && (double)anchor_q < reg.min_snp_q) atomicAdd(&cnt[K_COV * TP + al], 1);
                if (avail + 1 <= 61 && passes) {
                    if (refok_s[al]) atomicAdd(&cnt[((rev ? K_REV : K_FWD) + 5) * TP + al], 1);   // column I
                    atomicAdd(&cnt[K_INS * TP + al], 1);
                    vote = true;
                    vmeta = 1u | (rev ? 4u : 0u) | ((unsigned)avail << 4) | ((unsigned)al << 10);
                    voff = (unsigned)(rd.s0 - reg.seq_base + rfirst - 1);
                }
            }
            if (mine && op == OP_D && !(a.debug & 8)) {
                const int al = anchor - tile_lo;
                if (refok_s[al]) atomicAdd(&cnt[((rev ? K_REV : K_FWD) + 6) * TP + al], 1);       // column D, no quality test
                int avail = len + 1 < reg.ref_len - anchor ? len + 1 : reg.ref_len - anchor;
                if (avail < 0) avail = 0;
                if (avail + 1 <= 61) {
                    atomicAdd(&cnt[K_DEL * TP + al], 1);
                    vote = true;
                    vmeta = 2u | (rev ? 4u : 0u) | 8u | ((unsigned)avail << 4) | ((unsigned)al << 10);
                    voff = (unsigned)anchor;
                }
            }
            {   // allele votes wait in LDS for the verdict on their row; a tile with more than VCAP of them spills the rest
                const unsigned long long m = __ballot(vote);
                if (m) {
                    int base = 0;
                    const int leader = __ffsll((long long)m) - 1;
                    if (lane == leader) base = atomicAdd(&vcount, __popcll(m));
                    base = __builtin_amdgcn_readlane(base, leader);
                    const int slot = base + __popcll(m & ((1ull << lane) - 1ull));
                    const bool spill = vote && slot >= VCAP;
                    if (vote && !spill) vbuf[slot] = make_uint2(voff, vmeta);
                    if (__ballot(spill))
                        wave_append_vote(spill, Vote{(uint32_t)(tile_lo + (int)(vmeta >> 10)), (vmeta & 1023u) | ((uint32_t)region << 10), (int64_t)voff, 0},
                                         a.votes, &a.counters[CT_VOTES], a.vote_cap, lane);
                }
            }

            ENC_LAP(2);                               // per-operation section (inserts, deletions, votes)
            // -- the rows: a base that is a clean match (quality passes, equal to an A/C/G/T reference base) is already counted
            //    by its run; the '*' column of a deletion's rows (:541-551) is one unconditional add; everything else is queued
            const int strand = rev ? K_REV : K_FWD;
            // Which of the lane's rows need the full rules, as a bit per row; the wave's exceptions of the whole pass then enter
            // the queue with ONE prefix sum (round 3 pushed per row slot: eight ballots, rank computations, queue-length updates
            // and drain tests per pass, nearly all of them taken -- 5 % of the bases are exceptions, three per 64 rows)
            unsigned om = 0, okm = 0;
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int o = pl[u];
                const unsigned rb = (unsigned char)ref_s[o], b = (unsigned char)bv[u];
                const bool ref_ok = refok_s[o] != 0;
                const bool q_ok = qv[u] >= reg.qmin;
                atomicAdd(&cnt[(strand + 7) * TP + o], (is_d[u] && ref_ok) ? 1 : 0);
                const bool other = is_m[u] && !(q_ok && ref_ok && rb == b) && !(a.debug & 32);
                om |= other ? 1u << u : 0u;
                okm |= q_ok ? 1u << u : 0u;
            }
            if (__ballot(om != 0u)) {                     // (wave-uniform)
                const int mine_n = __popc(om);
                const int inc = wave_inclusive_sum(mine_n);
                const int total = wave_total(inc);
                if (qn + total <= XQ) {
                    int slot = qn + inc - mine_n;
#pragma unroll
                    for (int u = 0; u < UNR; ++u)
                        if ((om >> u) & 1u) {
                            xq_w[slot++] = (unsigned)pl[u] | ((unsigned)(unsigned char)bv[u] << 9) | (((okm >> u) & 1u) << 17) |
                                           (anchored[u] ? 1u << 18 : 0u) | (rev ? 1u << 19 : 0u);
                        }
                    qn += total;
                    __builtin_amdgcn_wave_barrier();
                    while (qn >= 64) {
                        drain(64);
                        const unsigned moved = lane < qn - 64 ? xq_w[64 + lane] : 0u;
                        __builtin_amdgcn_wave_barrier();
                        if (lane < qn - 64) xq_w[lane] = moved;
                        qn -= 64;
                        __builtin_amdgcn_wave_barrier();
                    }
                } else {
                    // more exceptions in one pass than the queue holds (a read that disagrees with the reference nearly
                    // everywhere): row slot by row slot, draining as it fills
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        const bool other = (om >> u) & 1u;
                        const unsigned long long m = __ballot(other);
                        if (m) {
                            const int slot = qn + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                            if (other)
                                xq_w[slot] = (unsigned)pl[u] | ((unsigned)(unsigned char)bv[u] << 9) | (((okm >> u) & 1u) << 17) |
                                             (anchored[u] ? 1u << 18 : 0u) | (rev ? 1u << 19 : 0u);
                            qn += __popcll(m);
                            __builtin_amdgcn_wave_barrier();
                            if (qn >= 64) {
                                drain(64);
                                const unsigned moved = lane < qn - 64 ? xq_w[64 + lane] : 0u;
                                __builtin_amdgcn_wave_barrier();
                                if (lane < qn - 64) xq_w[lane] = moved;
                                qn -= 64;
                                __builtin_amdgcn_wave_barrier();
                            }
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            ENC_LAP(3);                               // row phase (first use of the loaded bytes: their latency lands here)
            pos += total_r;
            ri += wave_total(qinc);
            if (pos > live_max) break;
        }
        rec = rec_next;
    }
    if (qn > 0) drain(qn);
    ENC_LAP(4);
    __syncthreads();
    ENC_LAP(5);                                       // waiting for the slowest wave of the tile

    // ---- the runs' share: prefix sums of the difference arrays = match-run coverage per strand and row, minus the anchoring
    //      last bases for the strand columns; the reference letter's column where the reference base is a letter
    {
        const int dF = tid < TP ? mcov[0][tid] : 0, dR = tid < TP ? mcov[1][tid] : 0;
        int sF = wave_inclusive_sum(dF), sR = wave_inclusive_sum(dR);
        if (lane == 63) {
            wtot[0][w] = sF;
            wtot[1][w] = sR;
        }
        __syncthreads();
        for (int k = 0; k < w; ++k) {
            sF += wtot[0][k];
            sR += wtot[1][k];
        }
        if (tid < TP) {
            const int an = anch[tid];
            cnt[K_COV * TP + tid] += sF + sR;
            cnt[K_FWD * TP + tid] += sF - (an & 0xffff);
            cnt[K_REV * TP + tid] += sR - (an >> 16);
            if (refok_s[tid]) {
                const unsigned ru = (unsigned char)ref_s[tid] & 0xDFu, ridx = (ru >> 1) & 3u;
                const int racgt = (int)(ridx ^ (ridx >> 1));
                cnt[(K_FWD + 1 + racgt) * TP + tid] += sF;
                cnt[(K_REV + 1 + racgt) * TP + tid] += sR;
            }
        }
    }
    __syncthreads();

    // ---- the tile is complete: per-position pass of generate_summary (:568-654), then one coalesced store --------
    const int idx = tile_lo + tid;
    int vals[MATF];
#pragma unroll
    for (int f = 0; f < MATF; ++f) vals[f] = 0;
    int cov = 0, n_snp = 0, n_ins = 0, n_del = 0, tab[8];
    const bool row = tid < TP && idx < L;
    if (row) {
        cov = cnt[K_COV * TP + tid];
        n_snp = cnt[K_SNP * TP + tid];
        n_ins = cnt[K_INS * TP + tid];
        n_del = cnt[K_DEL * TP + tid];
#pragma unroll
        for (int t = 0; t < 8; ++t) tab[t] = cnt[(K_TAB + t) * TP + tid];
        vals[0] = base_code(ref_s[tid]);
        vals[4] = -cnt[K_FWD * TP + tid];
        vals[15] = -cnt[K_REV * TP + tid];
#pragma unroll
        for (int s = 0; s < 7; ++s) {
            vals[8 + s] = -cnt[(K_FWD + 1 + s) * TP + tid];
            vals[19 + s] = -cnt[(K_REV + 1 + s) * TP + tid];
        }
    }
    __syncthreads();                               // every counter is in registers: the LDS becomes the output tile
    if (tid < TP) pass_s[tid] = 0;
    bool passes = false;
    SiteRec site{};
    if (row && !(a.debug & 4)) {
        const double c = cov > 1 ? (double)cov : 1.0;
        const bool s = (double)n_snp / c >= reg.snp_thr;
        const bool n = (double)n_ins / c >= reg.ins_thr;
        const bool d = (double)n_del / c >= reg.del_thr;
        passes = (s || n || d) && idx >= reg.cand_lo && idx <= reg.cand_hi && (double)cov >= reg.min_cov;
        if (a.targets != nullptr) passes = passes && a.targets[reg.row_base + idx] != 0;
        a.pass[reg.row_base + idx] = passes ? 1 : 0;
        if (FORM != TILE_PLAIN) a.depth[reg.row_base + idx] = cov;
        if (FORM == TILE_REFCONF) {
            // reads that show the reference letter and open no insert behind it speak for the reference; other letters, insert
            // anchors and deleted bases (not part of cov) against it.  vals[] hold the negated, still unclamped counters.
            const int code = vals[0];              // 1 .. 4: A C G T, 5: anything else
            int ref_col = 0;
#pragma unroll
            for (int s = 0; s < 4; ++s) ref_col = code == s + 1 ? -(vals[8 + s] + vals[19 + s]) : ref_col;
            const int ins = -(vals[12] + vals[23]), star = -(vals[14] + vals[25]);
            int n_ref = max(0, ref_col - ins);
            int n_alt = max(0, cov - ref_col) + min(ins, ref_col) + star;
            const long long n = (long long)n_ref + n_alt;
            if (n > REFCONF_SIDE - 1) {
                n_ref = (int)((100ll * n_ref + n - 1) / n);
                n_alt = 100 - n_ref;
            }
            a.gq[reg.row_base + idx] = code <= 4 ? a.gq_table[n_ref * REFCONF_SIDE + n_alt] : (uint8_t)0;
        }
        pass_s[tid] = passes ? 1 : 0;
        if (passes) {
            site.region = region;
            site.idx = idx;
            site.cov = cov;
            site.flags = (s ? 1 : 0) | (n ? 2 : 0) | (d ? 4 : 0);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                site.fwd[t] = tab[t];
                site.rev[t] = tab[4 + t];
            }
        }
#pragma unroll
        for (int col = 11; col < 25; ++col) vals[col] = max(-MAXC, min(MAXC, vals[col]));
    }
    if (tid < TP) {
#pragma unroll
        for (int f = 0; f < MATF; ++f) cnt[tid * MATF + f] = vals[f];
    }
    __syncthreads();
    const int n_rows = L + 1 - tile_lo < TP ? L + 1 - tile_lo : TP;
    const int n_out = n_rows * MATF;
    int* dst = a.mat + (reg.row_base + tile_lo) * (int64_t)MATF;          // 128-byte aligned: row_base % 16 == 0, tile_lo % 512 == 0
    if (!(a.debug & 2)) {
        for (int i = tid; i < n_out / 4; i += NT) reinterpret_cast<int4*>(dst)[i] = reinterpret_cast<const int4*>(cnt)[i];
        for (int i = (n_out & ~3) + tid; i < n_out; i += NT) dst[i] = cnt[i];
    }
    // The sites that passed and the votes of their rows (a few per cent of each) go to the region's lists, each vote with the
    // first bytes of its allele.  ONE update of the region's two counters per TILE: round 3 updated the site counter once per
    // passing row and the vote counter once per wave, and with ~200 tiles of a region at work on the same two words those
    // returning atomics, served one after the other by the L2, were a sixth of the kernel (tools/tile_ablation.sh).
    const int nv = (a.debug & 128) ? 0 : (vcount < VCAP ? vcount : VCAP);       // (VCAP == NT: one vote per thread)
    const uint2 pv = tid < nv ? vbuf[tid] : make_uint2(0, 0);
    const bool has = tid < nv && pass_s[pv.y >> 10];
    Vote v{(uint32_t)(tile_lo + (int)(pv.y >> 10)), (pv.y & 1023u) | ((uint32_t)region << 10), (int64_t)pv.x, 0};
    if (has) v.prefix = allele_prefix((pv.y & 8u) ? a.ref + reg.ref_off : a.seq + reg.seq_base, pv.x, (pv.y >> 4) & 63u);
    const unsigned long long sm = __ballot(passes), vm = __ballot(has);
    int s_at = 0, v_at = 0;
    if (lane == 0) {
        if (sm) s_at = atomicAdd(&s_out[0], __popcll(sm));
        if (vm) v_at = atomicAdd(&s_out[1], __popcll(vm));
    }
    s_at = __builtin_amdgcn_readfirstlane(s_at);      // (with every lane active: lane 0's value)
    v_at = __builtin_amdgcn_readfirstlane(v_at);
    __syncthreads();
    if (tid == 0) {
        if (s_out[0]) s_out[2] = atomicAdd(&a.region_counts[2 * region], s_out[0]);       // < L: one per row at most
        if (s_out[1]) s_out[3] = atomicAdd(&a.region_counts[2 * region + 1], s_out[1]);
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    if (passes) a.sites[reg.row_base + s_out[2] + s_at + __popcll(sm & below)] = site;
    if (has) a.votes_out[reg.vote_base + s_out[3] + v_at + __popcll(vm & below)] = v;
#ifdef PA_ENC_STAMP
    ENC_LAP(6);                                       // flush: prefix sums, per-position pass, store, votes
    if (lane == 0)
        for (int k = 0; k < 8; ++k) atomicAdd(&g_enc_cycles[k], lap_acc[k]);
#endif
}

// ---- per-position tracks: depth classes (pa_encoder_set_depth_bins), reference blocks (pa_encoder_set_ref_confidence) ----
// The rows of every region's candidate window [cand_lo, cand_hi] (clamped to [0, L - 1]; row L is never reported), each in
// the class of a value tile_count_kernel stored for it -- the depth track: the bin of the coverage; the reference-block track:
// the band of the GQ byte --, run-length encoded: one record per run head, in region and row order.  One workgroup per tile,
// one thread per row, launched twice around tile_offsets_kernel.  EMIT = false counts the tile's heads; EMIT = true computes
// the same flags again and writes every head at the tile's scanned offset plus its rank among the tile's heads.  A run's end
// is the next record's start in its region, or the window's end: the host derives it (fetch_track).  A row outside every
// target (targets != null) has the class TRACK_OFF_TARGET.  The two kernels share everything but what makes a head at a
// tile's first row and what a record carries beside its class: each says so where it decides.
constexpr int TRACK_CLASSES = 8;
constexpr int TRACK_OFF_TARGET = 255;
struct ClassBounds { int32_t n; int32_t lower[TRACK_CLASSES]; };     // lower[0] == 0 < lower[1] < ...; class k = [lower[k], lower[k + 1])

__device__ __forceinline__ int class_of(const ClassBounds& bounds, int value) {
    int k = 0;
#pragma unroll
    for (int j = 1; j < TRACK_CLASSES; ++j) k += (j < bounds.n && value >= bounds.lower[j]) ? 1 : 0;
    return k;
}

// the row of this thread: its region, the window's first row, the row in the region and in the batch, is it inside the window
struct TrackRow { int region, lo, idx; int64_t at; bool in; };
__device__ __forceinline__ TrackRow track_row(const RegRec* __restrict__ regions, const int32_t* __restrict__ tile_region) {
    TrackRow r;
    r.region = tile_region[blockIdx.x];
    const RegRec* reg = regions + r.region;
    r.lo = reg->cand_lo > 0 ? reg->cand_lo : 0;
    const int hi = reg->cand_hi < reg->L - 1 ? reg->cand_hi : reg->L - 1;
    r.idx = ((int)blockIdx.x - reg->tile0) * TP + (int)threadIdx.x;
    r.at = reg->row_base + r.idx;
    r.in = r.idx >= r.lo && r.idx <= hi;             // (idx <= L - 1: a row tile_count_kernel stored its values for)
    return r;
}
__device__ __forceinline__ bool row_on_target(const uint8_t* __restrict__ targets, int64_t at) { return targets == nullptr || targets[at] != 0; }

// the heads of a wave as a mask, their number where the tile's other waves read it behind the next barrier
__device__ __forceinline__ unsigned long long note_heads(bool head, int* wave_heads) {
    const unsigned long long hm = __ballot(head);
    if ((threadIdx.x & 63) == 0) wave_heads[threadIdx.x >> 6] = __popcll(hm);
    return hm;
}
// EMIT = false: the tile's head count for tile_offsets_kernel
__device__ __forceinline__ void store_tile_heads(const int* wave_heads, int* __restrict__ tile_heads) {
    if (threadIdx.x == 0) {
        int n = 0;
        for (int k = 0; k < TP / 64; ++k) n += wave_heads[k];
        tile_heads[blockIdx.x] = n;
    }
}
// the rank of this row's run among the tile's heads: heads at or before the row, less one (a head's own rank; its record's
// slot is the tile's scanned offset plus it)
__device__ __forceinline__ int head_rank(unsigned long long hm, const int* wave_heads) {
    int rank = __popcll(hm & ((2ull << (threadIdx.x & 63)) - 1ull)) - 1;
    for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) rank += wave_heads[k];
    return rank;
}

// The depth track.  The count pass also adds the tile's share of the region's totals (bases per bin, sum of depths: integers,
// so the order of the atomics does not show); a row outside every target adds nothing to them.
constexpr int DEPTH_TOTALS = TRACK_CLASSES + 1;     // per region: bases of bin 0 .. 7, sum of depths
struct DepthRun { int32_t region, row, bin; };

template <bool EMIT>
__global__ __launch_bounds__(TP) void depth_runs_kernel(const RegRec* __restrict__ regions, const int32_t* __restrict__ tile_region,
                                                        const int32_t* __restrict__ depth, const uint8_t* __restrict__ targets,
                                                        ClassBounds bins, int* __restrict__ tile_heads, const int* __restrict__ tile_off,
                                                        unsigned long long* __restrict__ totals, DepthRun* __restrict__ runs, int run_cap) {
    __shared__ uint8_t bin_s[TP];
    __shared__ int wave_heads[TP / 64];
    __shared__ int bases_s[TRACK_CLASSES];
    __shared__ unsigned long long sum_s;
    const int tid = threadIdx.x, lane = tid & 63;
    const TrackRow r = track_row(regions, tile_region);
    if (!EMIT && tid < TRACK_CLASSES) bases_s[tid] = 0;
    if (!EMIT && tid == 0) sum_s = 0;
    int d = 0, bin = TRACK_OFF_TARGET;
    bool on_target = false;
    if (r.in) {
        d = depth[r.at];
        on_target = row_on_target(targets, r.at);
        if (on_target) bin = class_of(bins, d);
    }
    bin_s[tid] = (uint8_t)bin;
    __syncthreads();
    // A run is ONE record, whatever tiles it crosses: a tile's first row looks back across the border, at the row in front
    // as the tile in front read it.
    bool head = false;
    if (r.in) {
        if (r.idx == r.lo) head = true;
        else if (tid > 0) head = bin_s[tid - 1] != bin;
        else head = (row_on_target(targets, r.at - 1) ? class_of(bins, depth[r.at - 1]) : TRACK_OFF_TARGET) != bin;
    }
    const unsigned long long hm = note_heads(head, wave_heads);
    if (!EMIT) {
        // the tile's share of the totals: per wave one LDS atomic per bin that occurs and one for the depths
        for (int k = 0; k < bins.n; ++k) {
            const unsigned long long m = __ballot(on_target && bin == k);
            if (m && lane == 0) atomicAdd(&bases_s[k], __popcll(m));
        }
        const long long dsum = wave_inclusive_sum64(on_target ? (long long)d : 0);
        if (lane == 63 && dsum) atomicAdd(&sum_s, (unsigned long long)dsum);
    }
    __syncthreads();
    if (!EMIT) {
        store_tile_heads(wave_heads, tile_heads);
        if (tid < TRACK_CLASSES && bases_s[tid]) atomicAdd(&totals[(size_t)r.region * DEPTH_TOTALS + tid], (unsigned long long)bases_s[tid]);
        if (tid == TRACK_CLASSES && sum_s) atomicAdd(&totals[(size_t)r.region * DEPTH_TOTALS + TRACK_CLASSES], sum_s);
    } else if (head) {
        const int slot = tile_off[blockIdx.x] + head_rank(hm, wave_heads);
        if (slot < run_cap) runs[slot] = DepthRun{r.region, r.idx, bin};      // past the capacity: the host emits again with room
    }
}

// The reference-block track: every record carries the smallest coverage and the smallest GQ of its rows.
struct RefBlock { int32_t region, row, band, min_dp, min_gq; };

template <bool EMIT>
__global__ __launch_bounds__(TP) void ref_blocks_kernel(const RegRec* __restrict__ regions, const int32_t* __restrict__ tile_region,
                                                        const int32_t* __restrict__ depth, const uint8_t* __restrict__ gq,
                                                        const uint8_t* __restrict__ targets, ClassBounds bands,
                                                        int* __restrict__ tile_heads, const int* __restrict__ tile_off,
                                                        RefBlock* __restrict__ blocks, int block_cap) {
    __shared__ uint8_t band_s[TP];
    __shared__ int wave_heads[TP / 64];
    __shared__ int min_dp_s[TP], min_gq_s[TP];       // per head of the tile, by rank (at most one head per row)
    const int tid = threadIdx.x;
    const TrackRow r = track_row(regions, tile_region);
    int d = 0, q = 0, band = TRACK_OFF_TARGET;
    if (r.in) {
        d = depth[r.at];
        q = gq[r.at];
        if (row_on_target(targets, r.at)) band = class_of(bands, q);
    }
    band_s[tid] = (uint8_t)band;
    if (EMIT) {
        min_dp_s[tid] = 0x7fffffff;
        min_gq_s[tid] = 0x7fffffff;
    }
    __syncthreads();
    // A run is one record PER TILE: a tile's first row inside the window is always a head, and the host joins touching records
    // of equal band with their minima (variant/RefConfidence.py merge_blocks, BlockTrack).  So every row of the window belongs
    // to a head of its own tile, and the minima are taken in LDS: atomicMin on the slot of the head's rank among the tile's
    // heads (a minimum does not depend on the order; no global atomic on the way to the output).
    const bool head = r.in && (r.idx == r.lo || tid == 0 || band_s[tid - 1] != band);
    const unsigned long long hm = note_heads(head, wave_heads);
    __syncthreads();
    if (!EMIT) {
        store_tile_heads(wave_heads, tile_heads);
        return;
    }
    const int rank = head_rank(hm, wave_heads);      // (>= 0 for every row of the window)
    if (r.in) {
        atomicMin(&min_dp_s[rank], d);
        atomicMin(&min_gq_s[rank], q);
    }
    __syncthreads();
    if (head) {
        const int slot = tile_off[blockIdx.x] + rank;
        if (slot < block_cap) blocks[slot] = RefBlock{r.region, r.idx, band, min_dp_s[rank], min_gq_s[rank]};   // past the capacity: emitted again with room
    }
}

// votes of the sites that passed the thresholds, compacted for the host
// (the number of votes is only known on the device: a fixed grid strides over counters[CT_VOTES] of them)
__global__ __launch_bounds__(256) void compact_votes_kernel(const Vote* __restrict__ votes, const int* __restrict__ counters, int cap,
                                                            const RegRec* __restrict__ regions, const uint8_t* __restrict__ pass,
                                                            const char* __restrict__ seq, const char* __restrict__ ref,
                                                            int* __restrict__ region_counts, Vote* __restrict__ out) {
    const int n = counters[CT_VOTES] < cap ? counters[CT_VOTES] : cap;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        Vote v = votes[i];
        const int r = (int)(v.meta >> 10);
        if (pass[regions[r].row_base + v.idx]) {
            v.prefix = allele_prefix((v.meta & 8u) ? ref + regions[r].ref_off : seq + regions[r].seq_base, (uint32_t)v.off, (v.meta >> 4) & 63u);
            out[regions[r].vote_base + atomicAdd(&region_counts[2 * r + 1], 1)] = v;
        }
    }
}

// The two region-sliced lists made dense for one copy to the host: region r's sites / votes move to the prefix sums of the
// counts before it (one workgroup per region; the counts of a batch are a few hundred integers).
// An insert allele of more than 8 bytes (its first 8 travel in the vote's prefix) is copied into a pool slot here and the vote's
// `off` becomes the slot: the host orders and names alleles without the reads, which in the packed form (pa_encoder_stage_packed)
// it never holds decoded.
__global__ __launch_bounds__(256) void pack_results_kernel(const RegRec* __restrict__ regions, const int* __restrict__ region_counts,
                                                           const SiteRec* __restrict__ sites, const Vote* __restrict__ votes,
                                                           SiteRec* __restrict__ sites_out, Vote* __restrict__ votes_out,
                                                           const char* __restrict__ seq, char* __restrict__ pool, int pool_cap,
                                                           int* __restrict__ counters) {
    __shared__ int off[2];
    const int r = blockIdx.x;
    if (threadIdx.x < 2) off[threadIdx.x] = 0;
    __syncthreads();
    int s = 0, v = 0;
    for (int q = threadIdx.x; q < r; q += 256) {
        s += region_counts[2 * q];
        v += region_counts[2 * q + 1];
    }
    if (s) atomicAdd(&off[0], s);
    if (v) atomicAdd(&off[1], v);
    __syncthreads();
    const int ns = region_counts[2 * r], nv = region_counts[2 * r + 1];
    const SiteRec* src_s = sites + regions[r].row_base;
    const Vote* src_v = votes + regions[r].vote_base;
    for (int i = threadIdx.x; i < ns; i += 256) sites_out[off[0] + i] = src_s[i];
    const char* rseq = seq + regions[r].seq_base;
    for (int i = threadIdx.x; i < nv; i += 256) {
        Vote v = src_v[i];
        const uint32_t len = (v.meta >> 4) & 63u;
        if (!(v.meta & 8u) && len > 8) {
            const int slot = atomicAdd(&counters[CT_POOL], 1);
            if (slot < pool_cap)
                for (uint32_t k = 0; k < len; ++k) pool[(size_t)slot * POOL_SLOT + k] = rseq[(size_t)v.off + k];
            v.off = slot;
        }
        votes_out[off[1] + i] = v;
    }
}

// one 64-lane workgroup per candidate: 33 x 26 = 858 cells
__device__ __forceinline__ void gather_window(const int* __restrict__ mat, const RegRec* __restrict__ regions,
                                              const CandDesc* __restrict__ cands, int c, int W, int F, int mid,
                                              int* __restrict__ out32, int8_t* __restrict__ out8) {
    const CandDesc cd = cands[c];
    const int L = regions[cd.region].L;
    const int* m = mat + regions[cd.region].row_base * MATF;
    const size_t base = (size_t)c * W * F;
    for (int e = threadIdx.x; e < W * F; e += 64) {
        const int r = e / F, f = e - r * F;
        const int row = cd.idx - mid + r;
        int v = (row >= 0 && row <= L && f < MATF) ? m[(size_t)row * MATF + f] : 0;
        if (r == mid) {
            if (f == cd.vcol) v = cd.vval;
            else if (f == cd.type + 4) v = cd.fwd;        // 5 / 6 / 7
            else if (f == cd.type + 15) v = cd.rev;       // 16 / 17 / 18
            else if (f == cd.neg_f || f == cd.neg_r) v = -v;
        } else if (r > mid && r <= cd.last) {
            if (f == 3) v = cd.vval;
            else if (f == 7) v = cd.fwd;
            else if (f == 18) v = cd.rev;
            else if (f == cd.star_f || f == cd.star_r) v = -v;
        }
        out32[base + e] = v;
        out8[base + e] = (int8_t)v;                        // two's-complement wrap, as numpy 1.22's int8 cast
    }
}
__global__ __launch_bounds__(64) void gather_windows_kernel(const int* __restrict__ mat, const RegRec* __restrict__ regions,
                                                            const CandDesc* __restrict__ cands, int W, int F, int mid,
                                                            int* __restrict__ out32, int8_t* __restrict__ out8) {
    gather_window(mat, regions, cands, (int)blockIdx.x, W, F, mid, out32, out8);
}

// ---- candidates enumerated on the device (pa_encoder_set_device_candidates) -------------------------------------------------
// What enumerate_region does on the host, between pack_results_kernel and the window gather, without a copy or a wait:
//   group_votes_kernel       one workgroup per region: every passing row learns its slot in the dense site list, the region's
//                            votes are counted per site and moved into one slice per site (a counting sort by site; the order
//                            of the slices and inside them is whatever the atomics give -- nothing below depends on it), the
//                            rare-alphabet entries are chained to their sites
//   enumerate_sites_kernel   one wavefront per site.  COUNT form: the site's votes into LDS, a bitonic sort under vote_less
//                            (candidates.h: the full order, tails in the reference / the pool included), written back sorted;
//                            runs of same_allele are tallied, the rule (candidates.h: accepted) decides, and the site's number of
//                            candidates and name bytes are added to its 512-row tile's totals.  WRITE form, after an exclusive scan
//                            of the tile totals (tile_offsets_kernel): the same walk over the sorted slice, each accepted allele
//                            written at tile offset + candidates of the tile's earlier rows + its rank in the site -- ascending
//                            rows of ascending regions, the host's order.  Two instances of each form: sites of at most 64
//                            votes (1.5 kB of LDS, nearly all of them), striding over the dense site list, and of 65 ..
//                            CAND_SITE_MAX votes (24 kB), striding over the list of such sites that group_votes_kernel
//                            leaves (a batch without one: its workgroups return at once).
//   gather_windows_n_kernel  gather_windows_kernel over a count that is only known on the device
// A call the kernels cannot take -- a site with more than CAND_SITE_MAX votes, or more than twelve rare letters -- raises
// CI_REFUSED: nothing is written and the host enumerates that call.  More candidates than the buffers hold: nothing is written,
// the host grows them and runs the call again.
constexpr int CAND_SITE_MAX = 1024;
enum { CI_SITES = 0, CI_REFUSED = 1, CI_LARGE = 2, CI_N = 4 };   // cinfo: passing sites of the batch | the call is refused | sites of more than 64 votes
struct SiteAux { int32_t v0, nv, fill, rare, nc, nb, pad0, pad1; };   // slice of the grouped votes, cursor, head of the rare chain (-1: none), candidates, name bytes
struct CandArgs {
    const RegRec* regions; const pa_cand::Rule* rules; int n_regions, n_tiles;
    const int* counters; const int* region_counts; const int* n_recs; int rec_cap, ovf_cap, pool_cap, vote_cap;
    const SiteRec* sites; const Vote* votes; Vote* grouped; const int4* ovf; int* rare_next;
    const char* ref; const char* pool; const uint8_t* pass; int* row_slot; SiteAux* aux; int* large;
    int* cinfo; int* tile_nc; int* tile_nb; const int* tile_c0; const int* tile_b0;
    int cand_cap, mid;
    CandDesc* cands; int64_t* positions; int32_t* depths; int32_t* freqs; char* names;
};
// the call will be run again with larger buffers, or fails: its lists are not complete (pool slots past pool_cap were never
// written), so nothing here reads them
__device__ __forceinline__ bool cand_call_void(const CandArgs& a) {
    return a.counters[CT_OVF] > a.ovf_cap || a.counters[CT_POOL] > a.pool_cap || *a.n_recs > a.rec_cap || a.counters[CT_ERR] > 0 ||
           a.counters[CT_VOTES] > a.vote_cap;
}
// ... or the device enumeration of it has nothing to write
__device__ __forceinline__ bool cand_no_output(const CandArgs& a) {
    return cand_call_void(a) || a.cinfo[CI_REFUSED] != 0 || a.tile_c0[a.n_tiles] > a.cand_cap;
}

__global__ __launch_bounds__(1024) void group_votes_kernel(CandArgs a) {
    if (cand_call_void(a)) return;
    __shared__ int off[3];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (tid < 3) off[tid] = 0;
    __syncthreads();
    int s = 0, v = 0;
    for (int q = tid; q < r; q += 1024) {
        s += a.region_counts[2 * q];
        v += a.region_counts[2 * q + 1];
    }
    if (s) atomicAdd(&off[0], s);
    if (v) atomicAdd(&off[1], v);
    __syncthreads();
    const int s_off = off[0], v_off = off[1];
    const int ns = a.region_counts[2 * r], nv = a.region_counts[2 * r + 1];
    const RegRec reg = a.regions[r];
    for (int i = tid; i < ns; i += 1024) {
        a.row_slot[reg.row_base + a.sites[s_off + i].idx] = s_off + i;
        a.aux[s_off + i] = SiteAux{0, 0, 0, -1, 0, 0, 0, 0};
    }
    __syncthreads();
    for (int j = tid; j < nv; j += 1024) atomicAdd(&a.aux[a.row_slot[reg.row_base + a.votes[v_off + j].idx]].nv, 1);
    // every region's workgroup reads the whole rare-alphabet list of the batch for its own entries: regions x entries, with a
    // handful of entries per batch (read letters outside ACGT on passing rows).  Piles rich in N would want a bucket per region.
    const int n_ovf = a.counters[CT_OVF];
    for (int k = tid; k < n_ovf; k += 1024) {
        const int4 o = a.ovf[k];
        if (o.w == r && o.x >= 0 && o.x < reg.L && a.pass[reg.row_base + o.x])
            a.rare_next[k] = atomicExch(&a.aux[a.row_slot[reg.row_base + o.x]].rare, k);
    }
    __syncthreads();
    for (int i = tid; i < ns; i += 1024) {
        const int n = atomicAdd(&a.aux[s_off + i].nv, 0);
        a.aux[s_off + i].v0 = v_off + atomicAdd(&off[2], n);      // (off[2] ends at nv: every vote of a region lies on a passing row)
        if (n > 64) a.large[atomicAdd(&a.cinfo[CI_LARGE], 1)] = s_off + i;   // (in no fixed order: a site's place in the output comes from its row)
    }
    __syncthreads();
    for (int j = tid; j < nv; j += 1024) {
        const Vote vt = a.votes[v_off + j];
        SiteAux* x = &a.aux[a.row_slot[reg.row_base + vt.idx]];
        a.grouped[x->v0 + atomicAdd(&x->fill, 1)] = vt;
    }
    if (r == (int)gridDim.x - 1 && tid == 0) a.cinfo[CI_SITES] = s_off + ns;
}

template <int CAP, bool WRITE>
__global__ __launch_bounds__(64) void enumerate_sites_kernel(CandArgs a) {
    if (WRITE ? cand_no_output(a) : cand_call_void(a)) return;
    __shared__ Vote sv[CAP];
    __shared__ pa_cand::SnpAllele s_snp[pa_cand::SNP_MAX];
    __shared__ int s_nsnp;
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int n_sites = a.cinfo[CAP == 64 ? CI_SITES : CI_LARGE];
    for (int q = blockIdx.x; q < n_sites; q += gridDim.x) {
        __syncthreads();                                   // the LDS of the previous site is free
        const int s = CAP == 64 ? q : a.large[q];
        const SiteAux aux = a.aux[s];
        const int nv = aux.nv;
        if (CAP == 64 && nv > 64) continue;                // the other instance's site
        if (nv > CAP) {
            if (!WRITE && lane == 0) a.cinfo[CI_REFUSED] = 1;
            continue;
        }
        if (WRITE && aux.nc == 0) continue;
        const SiteRec site = a.sites[s];
        const RegRec reg = a.regions[site.region];
        const pa_cand::Rule rule = a.rules[site.region];
        const AlleleSrc src{a.ref + reg.ref_off, a.pool};
        const int depth = pa_cand::clamp_count(site.cov);
        const char rb = site.idx < reg.ref_len ? src.reference[site.idx] : 'N';
        const int tile = reg.tile0 + site.idx / TP;
        // where the site's candidates and names go: the tile's offset + what the tile's earlier rows hold
        int c_at = 0, b_at = 0;
        if (WRITE) {
            for (int row = (site.idx / TP) * TP + lane; row < site.idx; row += 64)
                if (a.pass[reg.row_base + row]) {
                    const SiteAux& x = a.aux[a.row_slot[reg.row_base + row]];
                    c_at += x.nc;
                    b_at += x.nb;
                }
            c_at = a.tile_c0[tile] + wave_sum(c_at);
            b_at = a.tile_b0[tile] + wave_sum(b_at);
        }
        if (lane == 0) {
            int n = pa_cand::snp_from_site(site, s_snp);
            if (aux.rare >= 0) {
                bool full = false;
                for (int k = aux.rare; k >= 0; k = a.rare_next[k]) {
                    const int4 o = a.ovf[k];
                    if (!pa_cand::snp_merge(s_snp, n, (char)o.y, 1, o.z ? 0 : 1, o.z ? 1 : 0)) full = true;
                }
                pa_cand::snp_sort(s_snp, n);
                if (full && !WRITE) a.cinfo[CI_REFUSED] = 1;      // (which letters the host drops depends on its own order)
            }
            s_nsnp = n;
        }
        int P = 1;
        while (P < nv) P <<= 1;
        for (int k = lane; k < P; k += 64) sv[k] = k < nv ? a.grouped[aux.v0 + k] : Vote{0xffffffffu, 0u, 0, 0ull};   // (a row no site has: sorts last)
        __syncthreads();
        if (!WRITE && nv > 1) {
            for (int k2 = 2; k2 <= P; k2 <<= 1)
                for (int j = k2 >> 1; j > 0; j >>= 1) {
                    for (int i = lane; i < P; i += 64) {
                        const int m = i ^ j;
                        if (m > i) {
                            const Vote x = sv[i], y = sv[m];
                            if ((i & k2) == 0 ? vote_less(y, x, src) : vote_less(x, y, src)) {
                                sv[i] = y;
                                sv[m] = x;
                            }
                        }
                    }
                    __syncthreads();
                }
            for (int k = lane; k < nv; k += 64) a.grouped[aux.v0 + k] = sv[k];
        }
        // SNP alleles first, one per lane
        int n_c = 0, n_b = 0;
        {
            const bool acc = lane < s_nsnp && pa_cand::accepted(1, s_snp[lane < s_nsnp ? lane : 0].t, depth, site.flags, rule);
            const unsigned long long m = __ballot(acc);
            if (WRITE && acc) {
                const pa_cand::SnpAllele al = s_snp[lane];
                const int c = c_at + __popcll(m & below);
                char* name = a.names + b_at + 3 * __popcll(m & below);
                a.cands[c] = pa_cand::snp_desc(site.region, site.idx, rb, al.base, al.t);
                a.positions[c] = rule.region_start + site.idx;
                a.depths[c] = depth;
                a.freqs[c] = pa_cand::clamp_count(al.t.total);
                name[0] = '1';
                name[1] = al.base;
                name[2] = 0;
            }
            n_c = __popcll(m);
            n_b = 3 * n_c;
        }
        // then the runs of equal alleles in the sorted votes: the lane at a run's first vote tallies it
        for (int k0 = 0; k0 < nv; k0 += 64) {
            const int k = k0 + lane;
            Tally t{0, 0, 0};
            bool acc = false;
            int type = 0, alen = 0;
            if (k < nv && (k == 0 || !same_allele(sv[k], sv[k - 1], src))) {
                const Vote v = sv[k];
                for (int k1 = k; k1 < nv && (k1 == k || same_allele(sv[k1], v, src)); ++k1) {
                    t.total += 1;
                    ((sv[k1].meta & 4u) ? t.rev : t.fwd) += 1;
                }
                type = (v.meta & 3u) == 1u ? 2 : 3;
                alen = (int)pa_cand::allele_len(v);
                acc = pa_cand::accepted(type, t, depth, site.flags, rule);
            }
            const unsigned long long m = __ballot(acc);
            const int bytes = acc ? alen + 2 : 0;
            const int inc = wave_inclusive_sum(bytes);
            if (WRITE && acc) {
                const Vote v = sv[k];
                const int c = c_at + n_c + __popcll(m & below);
                char* name = a.names + b_at + n_b + inc - bytes;
                a.cands[c] = pa_cand::indel_desc(site.region, site.idx, rb, type, alen, t, a.mid, rule);
                a.positions[c] = rule.region_start + site.idx;
                a.depths[c] = depth;
                a.freqs[c] = pa_cand::clamp_count(t.total);
                name[0] = (char)('0' + type);
                pa_cand::copy_allele(name + 1, v, src);
                name[1 + alen] = 0;
            }
            n_c += __popcll(m);
            n_b += wave_total(inc);
        }
        if (!WRITE && lane == 0) {
            a.aux[s].nc = n_c;
            a.aux[s].nb = n_b;
            if (n_c) {
                atomicAdd(&a.tile_nc[tile], n_c);
                atomicAdd(&a.tile_nb[tile], n_b);
            }
        }
    }
}

// gather_windows_kernel for a count on the device: a fixed grid strides over the candidates
__global__ __launch_bounds__(64) void gather_windows_n_kernel(CandArgs a, const int* __restrict__ mat, int W, int F,
                                                              int* __restrict__ out32, int8_t* __restrict__ out8) {
    if (cand_no_output(a)) return;
    const int n = a.tile_c0[a.n_tiles];
    for (int c = blockIdx.x; c < n; c += gridDim.x) gather_window(mat, a.regions, a.cands, c, W, F, a.mid, out32, out8);
}

struct RegHost {
    pa_pileup p;
    pa_summary_params q;
    int L = 0;
    int64_t row_base = 0, seq_base = 0, op_base = 0, read_base = 0;
};

}  // namespace

namespace {

// CPUs this process may really use: the hardware's, cut by a cgroup quota (cgroup v2 cpu.max; the project's GPU boxes show 256
// logical CPUs and grant 16 -- 64 busy threads would each run at a quarter of the speed)
int usable_cpus() {
    int n = (int)std::thread::hardware_concurrency();
    if (n <= 0) n = 4;
    if (FILE* fh = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char quota[32] = {0};
        long long period = 0;
        if (fscanf(fh, "%31s %lld", quota, &period) == 2 && strcmp(quota, "max") != 0 && period > 0)
            n = std::min(n, std::max(1, (int)(atoll(quota) / period)));
        fclose(fh);
    }
    return n;
}

// worker threads that live as long as the encoder: the candidate enumeration of a batch is one short task per region
// (a few hundred microseconds of ordered maps and strings), and starting 16 threads per run cost more than the tasks
class RegionPool {
public:
    explicit RegionPool(int n) {
        for (int t = 0; t < n; ++t) threads_.emplace_back([this] { loop(); });
    }
    ~RegionPool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (std::thread& t : threads_) t.join();
    }
    int size() const { return (int)threads_.size(); }
    // fn(i) for i in [0, n): on the workers and on the caller; returns when all are done
    void run(int n, const std::function<void(int)>& fn) {
        {
            std::lock_guard<std::mutex> g(m_);
            fn_ = &fn;
            n_ = n;
            next_.store(0);
            left_ = n;
            ++epoch_;
        }
        cv_.notify_all();
        drain();
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [this] { return left_ == 0; });
        fn_ = nullptr;
    }

private:
    void drain() {
        for (;;) {
            const int i = next_.fetch_add(1);
            if (i >= n_) return;
            (*fn_)(i);
            std::lock_guard<std::mutex> g(m_);
            if (--left_ == 0) done_.notify_all();
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&] { return stop_ || epoch_ != seen; });
                if (stop_) return;
                seen = epoch_;
            }
            drain();
        }
    }
    std::vector<std::thread> threads_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* fn_ = nullptr;
    std::atomic<int> next_{0};
    int n_ = 0, left_ = 0;
    uint64_t epoch_ = 0;
    bool stop_ = false;
};

}  // namespace

struct pa_variant_batch {
    std::vector<RegHost> regs;
    int64_t total_bases = 0, total_ops = 0, total_reads = 0, total_rows = 0, total_ref = 0;
    int n_tiles = 0, W = 33, F = 26, mid = 16;
    int rec_cap = 0, ovf_cap = 0, pool_cap = 0;
    bool staged = false, packed = false;
    bool sampled = false;             // the staged packed batch has been through pa_enc::sample_pairs
    int64_t last_pairs = 0;           // (read, region) pairs of the last packed batch / chain run (in d_reads)
    DBuf d_seq, d_qual, d_ref, d_cig_op, d_cig_len, d_reads, d_regions, d_tile_region;
    // the tables of the staged batch as the kernels get them: the buffers above (pa_encoder_stage_batch) or slices of d_meta
    // (pa_encoder_stage_packed, one upload for all of them)
    const RegRec* p_regions = nullptr;
    const int32_t* p_tile_region = nullptr;
    const char* p_ref = nullptr;
    // packed form: the caller's arena as uploaded, the tables, what unpack_clip_kernel reports per region
    DBuf d_arena, d_meta, d_live, d_pool, d_comp, d_inf, d_walk;
    HBuf h_arena, h_meta, h_live, h_pool, h_comp, h_inf, h_walk;
    int64_t resident_bytes = 0;      // inflated bytes pa_encoder_inflate_bgzf left in d_arena (0: none)
    std::vector<int32_t> live;        // reads with a base inside each region (the reference's len(all_reads)) of the last run
    DBuf d_zero;                      // counters [CT_N] | per-region counts [2 n_regions] | tile_count [n_tiles] | tile_fill [n_tiles]: cleared per run
    DBuf d_targets;                   // verdicts of target_rows_kernel for the staged batch's rows (pa_encoder_set_targets)
    // The per-position tracks: depth classes (pa_encoder_set_depth_bins) and reference blocks (pa_encoder_set_ref_confidence).
    // What tile_count_kernel keeps for them, the coverage and the GQ byte of every row; per track the tiles' head counts (every
    // tile writes its own: nothing to clear), their scan, the records and the record count as the host gets it; of the last
    // run: was it made with the track's setting, its classes, its records; and the handle's counters (runs made with the
    // setting / runs whose records outgrew the buffer and were emitted a second time).  The depth track alone has totals:
    // [DEPTH_TOTALS x n_regions], cleared per run, and their host copy.
    struct RunTrack {
        DBuf d_heads, d_scan, d_recs;
        HBuf h_count;
        int64_t cap = 0, n = 0, calls = 0, overflows = 0;
        int classes = 0;
        bool on = false;
    };
    DBuf d_depth, d_gq, d_dtot;
    HBuf h_dtot;
    RunTrack depth, blocks;
    DBuf d_tile_off, d_sorted, d_mat, d_pass, d_sites, d_votes, d_votes_out, d_sites_dense, d_votes_dense, d_ovf, d_cands, d_img32, d_img8;
    HBuf h_counts, h_sites, h_votes;
    // candidates enumerated on the device (pa_encoder_set_device_candidates): the rules of the staged regions, the per-site and
    // per-row tables of group_votes_kernel, the tile totals and their scans, the results
    bool dev_cands = false;           // the switch
    bool dev_results = false;         // positions / depths / frequencies / names of the last run are still on the device
    bool dev_lists = false;           // d_pos / d_depths / d_freqs / d_names hold the last run's lists (enumerated there, or uploaded by selection_view)
    int cand_cap = 1024;              // candidates the result buffers hold (grown when a call has more)
    int64_t dev_calls = 0, host_calls = 0;     // calls enumerated on the device / on the host since the handle was created
    int64_t name_bytes = 0;
    DBuf d_rules, d_row_slot, d_aux, d_large, d_grouped, d_rare_next, d_czero, d_cscan, d_pos, d_depths, d_freqs, d_names;
    HBuf h_rules, h_cscan;
    // tables built on the device (pa_encoder_pack_records): where the last walk left its headers, the tables, the summary of
    // the last pack as the staging needs it
    struct { bool valid = false; bool mapped = false; size_t slots = 0, o_count = 0, o_flags = 0, o_out = 0, h_tail = 0;
             std::chrono::steady_clock::time_point t0; } walk;
    struct { bool valid = false; pa_device_pack sum{}; std::vector<int32_t> region_pairs, op_base; std::vector<int64_t> seq_base;
             int64_t on_device = 0, handed_back = 0; } pk;
    DBuf d_pk_hdr, d_pk_reads, d_pk_soff, d_pk_range, d_pk_pairs, d_pk_pair_read, d_pk_state;
    HBuf h_pk;
    std::unique_ptr<RegionPool> pool;
    int host_threads = 0;             // threads of the candidate enumeration: 0 = the default below, 1 = the calling thread alone
    // results of the last run
    int64_t n = 0;
    std::vector<int64_t> region_n;
    std::vector<int64_t> positions;
    std::vector<int32_t> depths, freqs;
    std::string names;
    double ms[15] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

void pa_variant_batch_free(pa_variant_batch* b) { delete b; }

namespace {

// candidates of one region in the reference's order (std::set<string> per site, region_summary.cpp:667-916)
struct RegionOut {
    std::vector<CandDesc> cands;
    std::vector<int64_t> positions;
    std::vector<int32_t> depths, freqs;
    std::string names;
};

// the order of the votes (vote_less, same_allele) and the rule (accepted, snp_desc, indel_desc): candidates.h, shared with
// enumerate_sites_kernel
using pa_cand::vote_less; using pa_cand::same_allele;

pa_cand::Rule region_rule(const RegHost& rh) {
    pa_cand::Rule q;
    q.support = rh.q.candidate_support_threshold;
    q.snp_freq = rh.q.snp_candidate_freq_threshold;
    q.indel_freq = rh.q.indel_candidate_freq_threshold;
    q.region_start = rh.p.region_start;
    q.skip_indels = rh.q.skip_indels;
    q.last_cap = rh.q.candidate_window_size - 1;
    return q;
}

void enumerate_region(const RegHost& rh, int region, int mid, const SiteRec* sites, size_t n_sites, const Vote* votes,
                      size_t n_votes, const int4* ovf, size_t n_ovf, const char* pool, RegionOut& out) {
    const pa_pileup& p = rh.p;
    const AlleleSrc src{p.reference, pool};
    const pa_cand::Rule rule = region_rule(rh);
    auto refc = [&](int64_t idx) { return idx >= 0 && idx < p.reference_len ? p.reference[idx] : 'N'; };
    std::map<int32_t, std::map<char, Tally>> rare;       // SNP alleles outside ACGT
    for (size_t k = 0; k < n_ovf; ++k) {
        Tally& t = rare[ovf[k].x][(char)ovf[k].y];
        t.total += 1;
        (ovf[k].z ? t.rev : t.fwd) += 1;
    }
    out.cands.reserve(2 * n_sites + 16);
    out.positions.reserve(2 * n_sites + 16);
    out.depths.reserve(2 * n_sites + 16);
    out.freqs.reserve(2 * n_sites + 16);
    out.names.reserve(8 * n_sites + 64);
    size_t vk = 0;                                        // votes are sorted by site, like the sites
    for (size_t si = 0; si < n_sites; ++si) {
        const SiteRec& s = sites[si];
        const int depth = std::min(s.cov, MAXC);
        const char rb = refc(s.idx);
        auto emit = [&](const std::string& key, const Tally& t, const CandDesc& d) {
            out.cands.push_back(d);
            out.positions.push_back(rule.region_start + s.idx);
            out.depths.push_back(depth);
            out.freqs.push_back(pa_cand::clamp_count(t.total));
            out.names += key;
            out.names.push_back('\0');
        };
        // SNP alleles: "1" + base, ordered by the raw base character (A C G T from the device's tallies are already in that
        // order; the rare alphabet, if any at this site, is merged in)
        pa_cand::SnpAllele snp[pa_cand::SNP_MAX];
        int n_snp = pa_cand::snp_from_site(s, snp);
        if (!rare.empty()) {
            const auto rit = rare.find(s.idx);
            if (rit != rare.end())
                for (const auto& kv : rit->second)      // (a letter the full site cannot take is dropped)
                    (void)pa_cand::snp_merge(snp, n_snp, kv.first, kv.second.total, kv.second.fwd, kv.second.rev);
            pa_cand::snp_sort(snp, n_snp);
        }
        for (int k = 0; k < n_snp; ++k) {
            if (!pa_cand::accepted(1, snp[k].t, depth, s.flags, rule)) continue;
            const char key[3] = {'1', snp[k].base, 0};
            emit(std::string(key, 2), snp[k].t, pa_cand::snp_desc(region, s.idx, rb, snp[k].base, snp[k].t));
        }
        while (vk < n_votes && (int32_t)votes[vk].idx < s.idx) ++vk;
        if (vk >= n_votes || (int32_t)votes[vk].idx != s.idx) continue;
        // allele keys "2" + anchor + inserted bases / "3" + deleted reference bases in std::map<std::string> order: the region's
        // votes arrive ordered by (site, type, allele bytes) -- see vote_less -- so equal keys are runs
        for (size_t k0 = vk; k0 < n_votes && (int32_t)votes[k0].idx == s.idx;) {
            size_t k1 = k0;
            Tally t{0, 0, 0};
            while (k1 < n_votes && same_allele(votes[k1], votes[k0], src)) {
                t.total += 1;
                ((votes[k1].meta & 4u) ? t.rev : t.fwd) += 1;
                ++k1;
            }
            const Vote& v = votes[k0];
            const int type = (v.meta & 3u) == 1u ? 2 : 3;
            const int alen = (int)pa_cand::allele_len(v);
            if (pa_cand::accepted(type, t, depth, s.flags, rule)) {
                std::string key(1 + (size_t)alen, (char)('0' + type));
                pa_cand::copy_allele(&key[1], v, src);
                emit(key, t, pa_cand::indel_desc(region, s.idx, rb, type, alen, t, mid, rule));
            }
            k0 = k1;
        }
        while (vk < n_votes && (int32_t)votes[vk].idx == s.idx) ++vk;
    }
}

// ---- staging: what the three entry points (stage_batch, the packed forms, pa_enc::unpack_packed_regions) share ----------------
const char* const BATCH_TOO_LARGE = "batch too large: more than 2^30 rows or 2^31 CIGAR operations / reads";

// a staging call, accepted or refused, leaves no earlier batch staged: first thing in each of them
void unstage(pa_encoder* e) {
    if (e && e->variant) e->variant->staged = false;
    if (e && e->variant) e->variant->depth.on = e->variant->blocks.on = false;      // (the last run's records speak of its regions)
}

struct RegionSums { int64_t rows = 0, ref = 0; int tiles = 0; };      // matrix rows, reference bytes and tiles of the regions so far

// One region of a batch, from its bounds, its reference length and its parameters: checked (the bounds; the parameters, which
// every region shares with q0, the batch's first), turned into its RegHost and its RegRec, and added to the sums.  seq_base /
// op_base / read_base: where its reads' bases, operations and read records start.  q == null (the polish chain, which brings no
// parameters and has matrices of its own): the record is zero but for L, and nothing else is written.
int region_pass(const pa_pileup& p, const pa_summary_params* q, const pa_summary_params* q0, int64_t seq_base, int64_t op_base,
                int64_t read_base, RegionSums& sums, RegHost* rh, RegRec& g) {
    if (p.region_end < p.region_start || p.region_end - p.region_start > (int64_t)1 << 28) return pa::set_error(PA_ERR_INVALID, "bad region");
    std::memset(&g, 0, sizeof(g));
    g.L = (int32_t)(p.region_end - p.region_start + 1);
    g.region_start = p.region_start;
    if (!q) return PA_OK;
    if (q->feature_size < 26 || q->candidate_window_size < 2 || q->candidate_window_size > 254)
        return pa::set_error(PA_ERR_INVALID, "feature_size must be >= 26 and 2 <= candidate_window_size <= 254");
    if (q->feature_size != q0->feature_size || q->candidate_window_size != q0->candidate_window_size)
        return pa::set_error(PA_ERR_INVALID, "one batch has one window size and one feature size");
    if (p.n_reads < 0 || p.reference_len < 0) return pa::set_error(PA_ERR_INVALID, "negative count");
    g.ref_off = sums.ref; g.row_base = sums.rows; g.seq_base = seq_base;
    g.ref_len = (int32_t)std::min<int64_t>(p.reference_len, 0x7fffffff);
    g.tile0 = sums.tiles; g.n_tiles = (g.L + 1 + TP - 1) / TP;
    auto row_of = [&](int64_t pos) { return (int32_t)std::max<int64_t>(-2, std::min<int64_t>(pos - p.region_start, 0x7ffffff0)); };
    g.cand_lo = row_of(q->candidate_region_start);
    g.cand_hi = row_of(q->candidate_region_end);
    // integer base quality Q passes `(double)Q >= min_snp_baseq` iff Q >= qmin
    g.qmin = std::isnan(q->min_snp_baseq) ? 256 : (q->min_snp_baseq <= 0 ? 0 : (q->min_snp_baseq > 255 ? 256 : (int)std::ceil(q->min_snp_baseq)));
    g.vote_base = (int32_t)op_base;
    g.min_snp_q = q->min_snp_baseq; g.min_indel_q = q->min_indel_baseq; g.min_cov = q->min_coverage_threshold;
    g.snp_thr = q->snp_freq_threshold; g.ins_thr = q->insert_freq_threshold; g.del_thr = q->delete_freq_threshold;
    rh->p = p; rh->q = *q; rh->L = g.L;
    rh->row_base = g.row_base; rh->seq_base = seq_base; rh->op_base = op_base; rh->read_base = read_base;
    sums.rows += (g.L + 1 + 15) & ~(int64_t)15;      // 16 rows x 104 B = 13 x 128 B: every tile store starts on a line
    sums.ref += p.reference_len;
    sums.tiles += g.n_tiles;
    if (sums.rows > ((int64_t)1 << 30)) return pa::set_error(PA_ERR_INVALID, BATCH_TOO_LARGE);
    return PA_OK;
}

// the sums of a finished region pass and the window of its regions' (shared) parameters
void set_geometry(pa_variant_batch& b, const RegionSums& sums, int32_t n_regions, const pa_summary_params* params) {
    b.total_rows = sums.rows; b.total_ref = sums.ref; b.n_tiles = sums.tiles;
    b.W = n_regions ? params[0].candidate_window_size + 1 : 33;
    b.F = n_regions ? params[0].feature_size : 26;
    b.mid = n_regions ? params[0].candidate_window_size / 2 : 16;
}

// records: a read enters a tile once per TP rows it spans, plus its first tile; reads with long deletions / skips span more
// rows than they have bases, so the kernels count what they could not store and the run is repeated with room
void set_record_caps(pa_variant_batch& b) {
    b.rec_cap = (int)std::min<int64_t>(0x7ffffff0, b.total_bases / TP + 2 * b.total_reads + 1024);
    b.ovf_cap = (int)std::min<int64_t>(0x7ffffff0, std::max<int64_t>(1 << 16, b.total_bases / 64));
    b.pool_cap = (int)std::min<int64_t>(0x7ffffff0, std::max<int64_t>(4096, b.total_ops / 64));
}

int stage_batch(pa_encoder* e, int32_t n_regions, const pa_pileup* pileups, const pa_summary_params* params) {
    unstage(e);
    if (!e || n_regions < 0 || (n_regions > 0 && (!pileups || !params))) return pa::set_error(PA_ERR_INVALID, "null argument");
    if (n_regions >= (1 << 22)) return pa::set_error(PA_ERR_INVALID, "more than 4194303 regions in one batch");
    ENC_HIP(hipSetDevice(e->device));
    if (!e->variant) e->variant = new pa_variant_batch();
    pa_variant_batch& b = *e->variant;
    b.ms[8] = b.ms[9] = 0;
    b.regs.assign((size_t)n_regions, RegHost());
    b.total_bases = b.total_ops = b.total_reads = 0;
    RegionSums sums;
    std::vector<RegRec> regrecs((size_t)n_regions);
    for (int r = 0; r < n_regions; ++r) {
        const pa_pileup& p = pileups[r];
        if (p.reference_len > 0x7fffffff || (p.n_reads > 0 && p.seq_offset[p.n_reads] > 0xffffffffll))
            return pa::set_error(PA_ERR_INVALID, "a region is limited to 2^32 read bases and 2^31 reference bases");
        const int rc = region_pass(p, &params[r], params, b.total_bases, b.total_ops, b.total_reads, sums, &b.regs[(size_t)r], regrecs[(size_t)r]);
        if (rc != PA_OK) return rc;
        b.total_reads += p.n_reads;
        b.total_bases += p.n_reads > 0 ? p.seq_offset[p.n_reads] : 0;
        b.total_ops += p.n_reads > 0 ? p.cigar_offset[p.n_reads] : 0;
        if (b.total_ops > 0x7ffffff0 || b.total_reads > 0x7ffffff0) return pa::set_error(PA_ERR_INVALID, BATCH_TOO_LARGE);
    }
    set_geometry(b, sums, n_regions, params);

    // read table
    std::vector<ReadRec> reads((size_t)b.total_reads);
    std::vector<int32_t> tile_region((size_t)b.n_tiles);
    for (int r = 0; r < n_regions; ++r) {
        const RegHost& rh = b.regs[(size_t)r];
        const pa_pileup& p = rh.p;
        for (int t = 0; t < regrecs[(size_t)r].n_tiles; ++t) tile_region[(size_t)(regrecs[(size_t)r].tile0 + t)] = r;
        for (int32_t k = 0; k < p.n_reads; ++k) {
            ReadRec& rd = reads[(size_t)(rh.read_base + k)];
            const int64_t slen = p.seq_offset[k + 1] - p.seq_offset[k], ncig = p.cigar_offset[k + 1] - p.cigar_offset[k];
            const int64_t row0 = p.read_pos[k] - p.region_start;
            if (slen < 0 || ncig < 0 || slen > 0x7ffffff0) return pa::set_error(PA_ERR_INVALID, "offsets of read " + std::to_string(k) + " are not ascending");
            rd.s0 = rh.seq_base + p.seq_offset[k];
            rd.c0 = (int32_t)(rh.op_base + p.cigar_offset[k]);
            rd.ncig = (int32_t)ncig;
            rd.slen = (int32_t)slen;
            // a read further than 2^30 rows from the region cannot reach it (CIGAR lengths are < 2^28 each, but their sum is
            // walked in int32): such a read is dropped here exactly as the walk would never touch a row
            rd.row0 = (int32_t)std::max<int64_t>(-(1 << 30), std::min<int64_t>(row0, 1 << 30));
            rd.region = r;
            rd.flags = (p.read_reverse[k] ? READ_REV : 0) | ((p.read_mapq[k] > 0 && row0 > -(1 << 30)) ? READ_MAPQ_OK : 0);
        }
    }

    hipStream_t st = e->stream;
    ENC_ALLOC(b.d_seq, (size_t)b.total_bases + 64);
    ENC_ALLOC(b.d_qual, (size_t)b.total_bases + 64);
    ENC_ALLOC(b.d_ref, (size_t)b.total_ref + 64);
    ENC_ALLOC(b.d_cig_op, (size_t)b.total_ops * 4 + 1024);      // the tile kernel issues 65-operation loads before it knows the read's end
    ENC_ALLOC(b.d_cig_len, (size_t)b.total_ops * 4 + 1024);
    ENC_ALLOC(b.d_reads, reads.size() * sizeof(ReadRec) + 64);
    ENC_ALLOC(b.d_regions, regrecs.size() * sizeof(RegRec) + 64);
    ENC_ALLOC(b.d_tile_region, tile_region.size() * 4 + 64);
    for (int r = 0; r < n_regions; ++r) {
        const RegHost& rh = b.regs[(size_t)r];
        const pa_pileup& p = rh.p;
        const int64_t nb = p.n_reads > 0 ? p.seq_offset[p.n_reads] : 0, no = p.n_reads > 0 ? p.cigar_offset[p.n_reads] : 0;
        if (nb > 0) {
            ENC_HIP(hipMemcpyAsync(b.d_seq.as<char>() + rh.seq_base, p.seq, (size_t)nb, hipMemcpyHostToDevice, st));
            ENC_HIP(hipMemcpyAsync(b.d_qual.as<char>() + rh.seq_base, p.qual, (size_t)nb, hipMemcpyHostToDevice, st));
        }
        if (no > 0) {
            ENC_HIP(hipMemcpyAsync(b.d_cig_op.as<int32_t>() + rh.op_base, p.cigar_op, (size_t)no * 4, hipMemcpyHostToDevice, st));
            ENC_HIP(hipMemcpyAsync(b.d_cig_len.as<int32_t>() + rh.op_base, p.cigar_len, (size_t)no * 4, hipMemcpyHostToDevice, st));
        }
        if (p.reference_len > 0)
            ENC_HIP(hipMemcpyAsync(b.d_ref.as<char>() + regrecs[(size_t)r].ref_off, p.reference, (size_t)p.reference_len, hipMemcpyHostToDevice, st));
    }
    if (!reads.empty()) ENC_HIP(hipMemcpyAsync(b.d_reads.p, reads.data(), reads.size() * sizeof(ReadRec), hipMemcpyHostToDevice, st));
    if (n_regions) {
        ENC_HIP(hipMemcpyAsync(b.d_regions.p, regrecs.data(), regrecs.size() * sizeof(RegRec), hipMemcpyHostToDevice, st));
        ENC_HIP(hipMemcpyAsync(b.d_tile_region.p, tile_region.data(), tile_region.size() * 4, hipMemcpyHostToDevice, st));
    }
    ENC_HIP(hipStreamSynchronize(st));            // the tables above are locals
    set_record_caps(b);
    b.p_regions = b.d_regions.as<RegRec>();
    b.p_tile_region = b.d_tile_region.as<int32_t>();
    b.p_ref = b.d_ref.as<char>();
    b.packed = false;
    b.live.assign((size_t)n_regions, 0);
    for (int r = 0; r < n_regions; ++r) b.live[(size_t)r] = pileups[r].n_reads;
    b.staged = true;
    return PA_OK;
}

// a packed read's slice(s) lie inside the arena: `CIGAR words | bases | qualities` from data_off, or the words there and
// `bases | qualities` from seq_off (pa_encoder_set_seq_offsets)
static bool packed_read_inside(const pa_packed_read& rd, int64_t seq_off, int64_t arena_bytes) {
    if (rd.n_cigar < 0 || rd.l_seq < 0 || rd.data_off < 0) return false;
    const int64_t ops_end = rd.data_off + 4ll * rd.n_cigar, bases = ((int64_t)rd.l_seq + 1) / 2 + rd.l_seq;
    if (seq_off < 0) return ops_end + bases <= arena_bytes;
    return ops_end <= arena_bytes && seq_off + bases <= arena_bytes;
}
// the table of pa_encoder_set_seq_offsets serves ONE staging call, accepted or refused: taken before anything else is checked
static std::vector<int64_t> take_seq_offsets(pa_encoder* e) {
    std::vector<int64_t> out;
    if (e) out.swap(e->seq_off);
    return out;
}

// Where a packed staging's page-locked block (and its copy on the device) keeps what it uploads:
// [RegRec x R][region_start x R][tile_region x tiles][PackedRead x reads][PairRec x pairs][base offsets x reads][reference bytes]
// -- the three tables are empty where pa_encoder_pack_records has built them on the device, tile_region and the reference for
// the polish chain
struct PackedBlock {
    size_t o_reg, o_start, o_tile, o_reads, o_pairs, o_soff, o_ref, bytes;
};
static PackedBlock lay_out_block(int32_t n_regions, int n_tiles, size_t reads_bytes, size_t pairs_bytes, size_t soff_bytes, int64_t ref_bytes) {
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    PackedBlock L{};
    L.o_start = up16(L.o_reg + (size_t)n_regions * sizeof(RegRec));
    L.o_tile = up16(L.o_start + (size_t)n_regions * 8);
    L.o_reads = up16(L.o_tile + (size_t)n_tiles * 4);
    L.o_pairs = up16(L.o_reads + reads_bytes);
    L.o_soff = up16(L.o_pairs + pairs_bytes);
    L.o_ref = up16(L.o_soff + soff_bytes);
    L.bytes = up16(L.o_ref + (size_t)ref_bytes + 64);
    return L;
}
// the tables unpack_clip_kernel reads, as device addresses (seq_off null: no read keeps its bases apart)
struct PackedTables {
    const PackedRead* reads; const PairRec* pairs; const int64_t* seq_off;
};
static PackedTables block_tables(const pa_variant_batch& b, const PackedBlock& L, bool with_seq_off) {
    const char* dm = b.d_meta.as<char>();
    return PackedTables{reinterpret_cast<const PackedRead*>(dm + L.o_reads), reinterpret_cast<const PairRec*>(dm + L.o_pairs),
                        with_seq_off ? reinterpret_cast<const int64_t*>(dm + L.o_soff) : nullptr};
}

// arena == NULL: the bytes pa_encoder_inflate_bgzf left on the device
static bool arena_is_resident(const uint8_t* arena, int32_t n_reads) { return arena == nullptr && n_reads > 0; }
static int check_resident(const pa_variant_batch& b, const uint8_t* arena, int32_t n_reads, int64_t arena_bytes) {
    if (arena_is_resident(arena, n_reads) && (b.resident_bytes <= 0 || arena_bytes > b.resident_bytes))
        return pa::set_error(PA_ERR_INVALID, "no arena given and no inflated span of that size resident on the device");
    return PA_OK;
}

// The (read, region) pairs of a packed batch, region by region: every pair's read checked (its index, its slices against the
// arena) and given its place -- the PairRec says where its clipped bases and operations go -- with the running sums per region
// left in seq_base / op_base [n_regions + 1].  Room: for the whole read (capped_by null: what is kept is known on the device
// only), or for what region r of capped_by[r].L rows can keep.  The clipped stretch of a read holds its aligned bases inside
// the region and the inserts between them: room for the whole read would be 10-50 kb per pair of a 1 kb region, so such a pair
// gets min(l_seq, 2 L + 64) bases and min(n_cigar, L + that + 2) operations (kept M / D / N operations each cover a row of the
// region, kept I / S ones a kept base); a pair that keeps more is reported as unsupported (h_live[n_regions + 1]) and the
// caller takes the host-clipped form.
static int walk_pairs(int32_t n_regions, const int32_t* region_pairs, const int32_t* pair_read, const pa_packed_read* reads, int32_t n_reads,
                      const std::vector<int64_t>& soff, int64_t arena_bytes, const RegRec* capped_by, PairRec* pairs, int64_t* seq_base,
                      int32_t* op_base) {
    int64_t bases = 0, ops = 0;
    seq_base[0] = 0;
    op_base[0] = 0;
    for (int r = 0; r < n_regions; ++r) {
        for (int32_t k = region_pairs[r]; k < region_pairs[r + 1]; ++k) {
            const int32_t ri = pair_read[k];
            if (ri < 0 || ri >= n_reads) return pa::set_error(PA_ERR_INVALID, "pair_read out of range");
            const pa_packed_read& rd = reads[ri];
            if (!packed_read_inside(rd, soff.empty() ? -1 : soff[(size_t)ri], arena_bytes))
                return pa::set_error(PA_ERR_INVALID, "packed read " + std::to_string(ri) + " lies outside the arena");
            const int64_t cap = capped_by ? std::min<int64_t>(rd.l_seq, 2ll * capped_by[r].L + 64) : 0;
            pairs[k] = PairRec{bases, ri, r, (int32_t)ops, (int32_t)cap};
            bases += pa_pack::base_room(capped_by ? cap : rd.l_seq);
            ops += capped_by ? std::min<int64_t>(rd.n_cigar, (int64_t)capped_by[r].L + cap + 2) : rd.n_cigar;
            if (ops > 0x7ffffff0) return pa::set_error(PA_ERR_INVALID, BATCH_TOO_LARGE);
        }
        seq_base[r + 1] = bases;
        op_base[r + 1] = (int32_t)ops;
    }
    return PA_OK;
}

// The block and the arena uploaded (one copy each; a resident arena stays where it is) and unpack_clip_kernel run over the
// tables `t`: the pairs' clipped reads in d_reads / d_seq / d_qual / d_cig_* (total_bases, total_ops: the room the pairs were
// given; extra_ops: more operation slots behind them, the polish chain's), what the kernel reports on its way to h_live.
// Nothing here waits for the device.  ev[6..8] bracket the uploads and the kernel for run_staged's ms[8] / ms[9]; the polish
// chain records them too, where nothing reads them (its call leaves no staged batch).
static int submit_unpack(pa_encoder* e, int32_t n_regions, int64_t n_pairs, const uint8_t* arena, int64_t arena_bytes, int32_t n_reads,
                         const PackedBlock& L, const PackedTables& t, int64_t total_bases, int64_t total_ops, int64_t extra_ops) {
    pa_variant_batch& b = *e->variant;
    const bool resident = arena_is_resident(arena, n_reads);
    hipStream_t st = e->stream;
    if (!resident) {
        ENC_ALLOC(b.d_arena, (size_t)arena_bytes + 256);
        b.resident_bytes = 0;
    }
    ENC_ALLOC(b.d_live, ((size_t)n_regions + 2) * 4);
    ENC_ALLOC(b.d_seq, (size_t)total_bases + 64);
    ENC_ALLOC(b.d_qual, (size_t)total_bases + 64);
    ENC_ALLOC(b.d_cig_op, (size_t)(total_ops + extra_ops) * 4 + 1024);
    ENC_ALLOC(b.d_cig_len, (size_t)(total_ops + extra_ops) * 4 + 1024);
    ENC_ALLOC(b.d_reads, (size_t)n_pairs * sizeof(ReadRec) + 64);
    ENC_HIP(hipEventRecord(e->ev[6], st));
    if (arena_bytes > 0 && !resident) ENC_HIP(hipMemcpyAsync(b.d_arena.p, arena, (size_t)arena_bytes, hipMemcpyHostToDevice, st));
    ENC_HIP(hipMemcpyAsync(b.d_meta.p, b.h_meta.p, L.bytes, hipMemcpyHostToDevice, st));
    ENC_HIP(hipMemsetAsync(b.d_live.p, 0, ((size_t)n_regions + 2) * 4, st));
    ENC_HIP(hipEventRecord(e->ev[7], st));
    const char* dm = b.d_meta.as<char>();
    b.p_regions = reinterpret_cast<const RegRec*>(dm + L.o_reg);
    b.p_tile_region = reinterpret_cast<const int32_t*>(dm + L.o_tile);
    b.p_ref = dm + L.o_ref;
    if (n_pairs > 0) {
        UnpackArgs ua;
        ua.pairs = t.pairs; ua.n_pairs = (int)n_pairs; ua.preads = t.reads; ua.seq_off = t.seq_off;
        ua.regions = b.p_regions; ua.region_start = reinterpret_cast<const int64_t*>(dm + L.o_start); ua.n_regions = n_regions;
        ua.arena = b.d_arena.as<uint8_t>();
        ua.reads = b.d_reads.as<ReadRec>(); ua.cigar_op = b.d_cig_op.as<int32_t>(); ua.cigar_len = b.d_cig_len.as<int32_t>();
        ua.seq = b.d_seq.as<char>(); ua.qual = b.d_qual.as<uint8_t>(); ua.live = b.d_live.as<int>();
        hipLaunchKernelGGL(unpack_clip_kernel, dim3((unsigned)((n_pairs + 3) / 4)), dim3(256), 0, st, ua);
        ENC_HIP(hipGetLastError());
    }
    ENC_HIP(hipEventRecord(e->ev[8], st));
    ENC_HIP(hipMemcpyAsync(b.h_live.p, b.d_live.p, ((size_t)n_regions + 2) * 4, hipMemcpyDeviceToHost, st));
    b.last_pairs = n_pairs;
    return PA_OK;
}

// A packed staging, whoever built the tables.  Host tables (reads, pair_read; soff: the base offsets set for the call) travel
// in the block, and every pair is walked here.  device_tables: those pa_encoder_pack_records left on the device -- it has
// placed the pairs, checked every read against the span and summed the same offsets (b.pk), so the block carries the regions
// and the reference only.  One pass over the regions, the block laid out from its sums, the pairs placed, the region records
// put into the block with where their reads' bases and operations start, then the submission: nothing here waits for the device.
static int stage_packed_tables(pa_encoder* e, int32_t n_regions, const pa_packed_region* regions, const pa_summary_params* params,
                               const uint8_t* arena, int64_t arena_bytes, const pa_packed_read* reads, int32_t n_reads,
                               const int32_t* pair_read, const int32_t* region_pairs, const std::vector<int64_t>& soff,
                               bool device_tables) {
    if (n_regions >= (1 << 22)) return pa::set_error(PA_ERR_INVALID, "more than 4194303 regions in one batch");
    ENC_HIP(hipSetDevice(e->device));
    if (!e->variant) e->variant = new pa_variant_batch();
    pa_variant_batch& b = *e->variant;
    int rc = check_resident(b, arena, n_reads, arena_bytes);
    if (rc != PA_OK) return rc;
    b.ms[8] = b.ms[9] = 0;
    b.regs.assign((size_t)n_regions, RegHost());
    b.total_bases = b.total_ops = b.total_reads = 0;
    const int64_t n_pairs = n_regions ? region_pairs[n_regions] : 0;
    if (n_pairs < 0 || (n_regions && region_pairs[0] != 0)) return pa::set_error(PA_ERR_INVALID, "region_pairs must start at 0 and ascend");
    RegionSums sums;
    std::vector<RegRec> regrecs((size_t)n_regions);      // (kept here until the block exists: its layout needs the sums)
    for (int r = 0; r < n_regions; ++r) {
        if (regions[r].reference_len > 0x7fffffff) return pa::set_error(PA_ERR_INVALID, "negative count");      // (this form's words for it)
        pa_pileup p{};
        p.region_start = regions[r].region_start; p.region_end = regions[r].region_end;
        p.reference = regions[r].reference; p.reference_len = regions[r].reference_len;
        p.n_reads = region_pairs[r + 1] < region_pairs[r] ? -1 : region_pairs[r + 1] - region_pairs[r];      // (descending: a negative count)
        rc = region_pass(p, &params[r], params, 0, 0, region_pairs[r], sums, &b.regs[(size_t)r], regrecs[(size_t)r]);
        if (rc != PA_OK) return rc;
    }
    set_geometry(b, sums, n_regions, params);
    const PackedBlock L = lay_out_block(n_regions, b.n_tiles, device_tables ? 0 : (size_t)n_reads * sizeof(PackedRead),
                                        device_tables ? 0 : (size_t)n_pairs * sizeof(PairRec), soff.size() * 8, b.total_ref);
    if (!b.h_meta.ensure(L.bytes) || !b.h_live.ensure(((size_t)n_regions + 2) * 4)) return pa::set_error(PA_ERR_HIP, "hipHostMalloc failed");
    ENC_ALLOC(b.d_meta, L.bytes);
    char* hm = b.h_meta.as<char>();
    std::vector<int64_t> walked_bases;
    std::vector<int32_t> walked_ops;
    const int64_t* seq_base = b.pk.seq_base.data();
    const int32_t* op_base = b.pk.op_base.data();
    PackedTables t{b.d_pk_reads.as<PackedRead>(), b.d_pk_pairs.as<PairRec>(), b.pk.sum.n_split > 0 ? b.d_pk_soff.as<int64_t>() : nullptr};
    if (!device_tables) {
        if (n_reads) std::memcpy(hm + L.o_reads, reads, (size_t)n_reads * sizeof(PackedRead));
        if (!soff.empty()) std::memcpy(hm + L.o_soff, soff.data(), soff.size() * 8);
        walked_bases.resize((size_t)n_regions + 1);
        walked_ops.resize((size_t)n_regions + 1);
        rc = walk_pairs(n_regions, region_pairs, pair_read, reads, n_reads, soff, arena_bytes, nullptr, reinterpret_cast<PairRec*>(hm + L.o_pairs),
                        walked_bases.data(), walked_ops.data());
        if (rc != PA_OK) return rc;
        seq_base = walked_bases.data();
        op_base = walked_ops.data();
        t = block_tables(b, L, !soff.empty());
    }
    int64_t* rstart = reinterpret_cast<int64_t*>(hm + L.o_start);
    int32_t* tile_region = reinterpret_cast<int32_t*>(hm + L.o_tile);
    for (int r = 0; r < n_regions; ++r) {
        if (seq_base[r + 1] < seq_base[r] || op_base[r + 1] < op_base[r] || op_base[r + 1] > 0x7ffffff0)
            return pa::set_error(PA_ERR_INVALID, BATCH_TOO_LARGE);
        if (seq_base[r + 1] - seq_base[r] > 0xffffff00ll) return pa::set_error(PA_ERR_INVALID, "a region is limited to 2^32 read bases");
        RegHost& rh = b.regs[(size_t)r];
        RegRec& g = regrecs[(size_t)r];
        g.seq_base = rh.seq_base = seq_base[r];
        g.vote_base = op_base[r];
        rh.op_base = op_base[r];
        rstart[r] = rh.p.region_start;
        for (int t2 = 0; t2 < g.n_tiles; ++t2) tile_region[g.tile0 + t2] = r;
        if (rh.p.reference_len > 0) std::memcpy(hm + L.o_ref + g.ref_off, rh.p.reference, (size_t)rh.p.reference_len);
    }
    if (n_regions) std::memcpy(hm + L.o_reg, regrecs.data(), (size_t)n_regions * sizeof(RegRec));
    b.total_bases = seq_base[n_regions];
    b.total_ops = op_base[n_regions];
    b.total_reads = n_pairs;
    rc = submit_unpack(e, n_regions, n_pairs, arena, arena_bytes, n_reads, L, t, b.total_bases, b.total_ops, 0);
    if (rc != PA_OK) return rc;
    set_record_caps(b);
    b.live.assign((size_t)n_regions, 0);
    b.packed = true;
    b.sampled = false;
    b.staged = true;
    return PA_OK;
}

// The packed form of a batch (include/pepper_amd_encoder.h) from host tables
int stage_packed(pa_encoder* e, int32_t n_regions, const pa_packed_region* regions, const pa_summary_params* params,
                 const uint8_t* arena, int64_t arena_bytes, const pa_packed_read* reads, int32_t n_reads, const int32_t* pair_read,
                 const int32_t* region_pairs) {
    const std::vector<int64_t> soff = take_seq_offsets(e);
    unstage(e);
    if (!e || n_regions < 0 || (n_regions > 0 && (!regions || !params || !region_pairs)) || arena_bytes < 0 || n_reads < 0 ||
        (n_reads > 0 && (!reads || !pair_read)))
        return pa::set_error(PA_ERR_INVALID, "null argument");
    if (!soff.empty() && (int64_t)soff.size() != n_reads)
        return pa::set_error(PA_ERR_INVALID, "the base offsets set for this call are not one per packed read");
    return stage_packed_tables(e, n_regions, regions, params, arena, arena_bytes, reads, n_reads, pair_read, region_pairs, soff, false);
}

// The same batch over the tables pa_encoder_pack_records left on the device
static int stage_packed_device(pa_encoder* e, int32_t n_regions, const pa_packed_region* regions, const pa_summary_params* params) {
    take_seq_offsets(e);                      // (a table set for this call has nothing to say about the device's reads)
    unstage(e);
    pa_variant_batch& b = *e->variant;
    if (n_regions < 0 || (n_regions > 0 && (!regions || !params))) return pa::set_error(PA_ERR_INVALID, "null argument");
    // (no read: nothing is dereferenced, and the staging takes no arena -- as the host-table form is called for such a run)
    const int32_t n_reads = b.pk.sum.n_reads;
    return stage_packed_tables(e, n_regions, regions, params, nullptr, n_reads > 0 ? b.resident_bytes : 0, nullptr, n_reads, nullptr,
                               b.pk.region_pairs.data(), std::vector<int64_t>(), true);
}

// ---- a run of the staged batch, in steps (run_staged below calls them in this order) ----------------------------------------
// what the steps share: the sizes the staged batch fixes, the slices of d_zero and the page-locked copy of the counters
struct RunShape {
    int n_regions = 0, vote_cap = 0;
    size_t n_zero = 0, n_czero = 0, n_cscan = 0;
    bool dev = false;                                           // candidates enumerated by the kernels (the handle's switch)
    int *counters = nullptr, *region_counts = nullptr, *tile_count = nullptr, *tile_fill = nullptr;
    int* host_counters = nullptr;                               // [CT_N] | per-region counts | records
};

// the workspaces sized by the batch (those sized by the record caps belong to the attempts); with the switch on, the rule of
// every region and the tables of the candidate kernels too
int size_workspaces(pa_encoder* e, RunShape& w) {
    pa_variant_batch& b = *e->variant;
    const int n_regions = w.n_regions = (int)b.regs.size();
    w.vote_cap = (int)std::min<int64_t>(b.total_ops + 1, 0x7ffffff0);
    w.n_zero = (size_t)CT_N + 2 * (size_t)n_regions + 2 * (size_t)b.n_tiles;
    w.n_czero = (size_t)CI_N + 2 * (size_t)b.n_tiles;
    w.n_cscan = 2 * ((size_t)b.n_tiles + 1);
    w.dev = b.dev_cands;
    ENC_ALLOC(b.d_zero, w.n_zero * 4);
    ENC_ALLOC(b.d_tile_off, ((size_t)b.n_tiles + 1) * 4);
    ENC_ALLOC(b.d_mat, (size_t)b.total_rows * MATF * 4 + 64);
    ENC_ALLOC(b.d_pass, (size_t)b.total_rows + 64);
    ENC_ALLOC(b.d_sites, (size_t)b.total_rows * sizeof(SiteRec));
    ENC_ALLOC(b.d_votes, (size_t)w.vote_cap * sizeof(Vote));
    ENC_ALLOC(b.d_votes_out, (size_t)w.vote_cap * sizeof(Vote));
    ENC_ALLOC(b.d_sites_dense, (size_t)b.total_rows * sizeof(SiteRec));
    ENC_ALLOC(b.d_votes_dense, (size_t)w.vote_cap * sizeof(Vote));
    if (!b.h_counts.ensure(((size_t)CT_N + 2 * (size_t)n_regions + 1) * 4)) return pa::set_error(PA_ERR_HIP, "hipHostMalloc failed");
    w.host_counters = b.h_counts.as<int>();
    w.counters = b.d_zero.as<int>();
    w.region_counts = w.counters + CT_N;
    w.tile_count = w.region_counts + 2 * n_regions;
    w.tile_fill = w.tile_count + b.n_tiles;
    if (!w.dev) return PA_OK;
    if (!b.h_rules.ensure((size_t)n_regions * sizeof(pa_cand::Rule)) || !b.h_cscan.ensure((w.n_cscan + CI_N) * 4))
        return pa::set_error(PA_ERR_HIP, "hipHostMalloc failed");
    for (int r = 0; r < n_regions; ++r) b.h_rules.as<pa_cand::Rule>()[r] = region_rule(b.regs[(size_t)r]);
    ENC_ALLOC(b.d_rules, (size_t)n_regions * sizeof(pa_cand::Rule));
    ENC_ALLOC(b.d_row_slot, (size_t)b.total_rows * 4 + 64);
    ENC_ALLOC(b.d_aux, (size_t)b.total_rows * sizeof(SiteAux) + 64);
    ENC_ALLOC(b.d_large, (size_t)b.total_rows * 4 + 64);         // (a row holds at most one site)
    ENC_ALLOC(b.d_grouped, (size_t)w.vote_cap * sizeof(Vote));
    ENC_ALLOC(b.d_czero, w.n_czero * 4);
    ENC_ALLOC(b.d_cscan, w.n_cscan * 4);
    return PA_OK;
}

// one attempt's count kernels: the records of every tile, tile_count_kernel, the votes compacted and the lists packed
int submit_counts(pa_encoder* e, const RunShape& w) {
    pa_variant_batch& b = *e->variant;
    hipStream_t st = e->stream;
    ENC_ALLOC(b.d_sorted, (size_t)b.rec_cap * sizeof(TileRec));
    ENC_ALLOC(b.d_ovf, (size_t)b.ovf_cap * sizeof(int4));
    ENC_ALLOC(b.d_pool, (size_t)b.pool_cap * POOL_SLOT);
    ENC_HIP(hipMemsetAsync(b.d_zero.p, 0, w.n_zero * 4, st));
    const uint8_t* targets = nullptr;             // a table is set: the verdict of every row, in front of the timed kernels
    if (e->n_targets > 0) {
        ENC_ALLOC(b.d_targets, (size_t)b.total_rows + 64);
        const int64_t* tab = e->d_target_table.as<int64_t>();
        hipLaunchKernelGGL(target_rows_kernel, dim3((unsigned)b.n_tiles), dim3(TRT), 0, st, b.p_regions, b.p_tile_region, tab,
                           tab + e->n_targets, e->n_targets, b.d_targets.as<uint8_t>());
        targets = b.d_targets.as<uint8_t>();
    }
    ENC_HIP(hipEventRecord(e->ev[0], st));
    const dim3 seg_grid((unsigned)((b.total_reads + 3) / 4));
    if (b.total_reads > 0)
        hipLaunchKernelGGL(segment_reads_kernel<false>, seg_grid, dim3(256), 0, st, b.d_reads.as<ReadRec>(), (int)b.total_reads,
                           b.p_regions, b.d_cig_op.as<int32_t>(), b.d_cig_len.as<int32_t>(), w.tile_count,
                           (const int*)nullptr, (int*)nullptr, (TileRec*)nullptr, 0);
    hipLaunchKernelGGL(tile_offsets_kernel, dim3(1), dim3(1024), 0, st, w.tile_count, b.n_tiles, b.d_tile_off.as<int>());
    if (b.total_reads > 0)
        hipLaunchKernelGGL(segment_reads_kernel<true>, seg_grid, dim3(256), 0, st, b.d_reads.as<ReadRec>(), (int)b.total_reads,
                           b.p_regions, b.d_cig_op.as<int32_t>(), b.d_cig_len.as<int32_t>(), w.tile_count,
                           b.d_tile_off.as<int>(), w.tile_fill, b.d_sorted.as<TileRec>(), b.rec_cap);
    ENC_HIP(hipEventRecord(e->ev[1], st));
    TileArgs ta;
    ta.reads = b.d_reads.as<ReadRec>(); ta.regions = b.p_regions; ta.tile_region = b.p_tile_region;
    ta.cigar_op = b.d_cig_op.as<int32_t>(); ta.cigar_len = b.d_cig_len.as<int32_t>();
    ta.seq = b.d_seq.as<char>(); ta.qual = b.d_qual.as<uint8_t>(); ta.ref = b.p_ref;
    ta.recs = b.d_sorted.as<TileRec>(); ta.tile_off = b.d_tile_off.as<int>(); ta.rec_cap = b.rec_cap;
    ta.mat = b.d_mat.as<int>(); ta.pass = b.d_pass.as<uint8_t>(); ta.sites = b.d_sites.as<SiteRec>();
    ta.votes = b.d_votes.as<Vote>(); ta.votes_out = b.d_votes_out.as<Vote>(); ta.vote_cap = w.vote_cap;
    ta.ovf = b.d_ovf.as<int4>(); ta.ovf_cap = b.ovf_cap; ta.counters = w.counters; ta.region_counts = w.region_counts;
    static const int tile_debug = [] { const char* e = getenv("PA_TILE_DEBUG"); return e ? atoi(e) : 0; }();
    ta.debug = tile_debug;
    ta.targets = targets;
    ta.depth = nullptr;                            // depth bins set: the tile kernel keeps every row's coverage for depth_runs_kernel
    ta.gq = nullptr;                               // a reference-confidence table set: the coverage and the GQ byte for ref_blocks_kernel
    ta.gq_table = nullptr;
    if (e->depth_bins.n > 0 || e->ref_bands.n > 0) {
        ENC_ALLOC(b.d_depth, (size_t)b.total_rows * 4 + 64);
        ta.depth = b.d_depth.as<int32_t>();
    }
    if (e->ref_bands.n > 0) {
        ENC_ALLOC(b.d_gq, (size_t)b.total_rows + 64);
        ta.gq = b.d_gq.as<uint8_t>();
        ta.gq_table = e->d_gq_table.as<uint8_t>();
    }
    if (ta.gq != nullptr) hipLaunchKernelGGL(tile_count_kernel<TILE_REFCONF>, dim3((unsigned)b.n_tiles), dim3(NT), 0, st, ta);
    else if (ta.depth != nullptr) hipLaunchKernelGGL(tile_count_kernel<TILE_DEPTH>, dim3((unsigned)b.n_tiles), dim3(NT), 0, st, ta);
    else hipLaunchKernelGGL(tile_count_kernel<TILE_PLAIN>, dim3((unsigned)b.n_tiles), dim3(NT), 0, st, ta);
    ENC_HIP(hipEventRecord(e->ev[2], st));
    hipLaunchKernelGGL(compact_votes_kernel, dim3((unsigned)std::min(2048, (w.vote_cap + 255) / 256)), dim3(256), 0, st, b.d_votes.as<Vote>(),
                       w.counters, w.vote_cap, b.p_regions, b.d_pass.as<uint8_t>(), b.d_seq.as<char>(), b.p_ref, w.region_counts,
                       b.d_votes_out.as<Vote>());
    hipLaunchKernelGGL(pack_results_kernel, dim3((unsigned)w.n_regions), dim3(256), 0, st, b.p_regions, w.region_counts,
                       b.d_sites.as<SiteRec>(), b.d_votes_out.as<Vote>(), b.d_sites_dense.as<SiteRec>(), b.d_votes_dense.as<Vote>(),
                       b.d_seq.as<char>(), b.d_pool.as<char>(), b.pool_cap, w.counters);
    ENC_HIP(hipEventRecord(e->ev[3], st));
    ENC_HIP(hipGetLastError());
    return PA_OK;
}

// ---- the per-position tracks behind everything else of the submission: the depth classes, then the reference blocks ---------
using RunTrack = pa_variant_batch::RunTrack;
struct TrackSlots { int ev, ms; size_t rec_bytes; };     // events ev, ev + 1 around the track's kernels, their time in ms[ms]; a record
constexpr TrackSlots DEPTH_SLOTS{12, 13, sizeof(DepthRun)}, BLOCK_SLOTS{14, 14, sizeof(RefBlock)};

ClassBounds track_bounds(const RunTrack& t, const pa_track_setting& set) {
    ClassBounds bounds;
    bounds.n = t.classes;
    for (int k = 0; k < TRACK_CLASSES; ++k) bounds.lower[k] = set.lower[k];
    return bounds;
}

// the count pass (first the totals cleared: a failure shows at the submission's hipGetLastError) or the emit pass of each track
void launch_depth_runs(pa_encoder* e, bool emit) {
    pa_variant_batch& b = *e->variant;
    if (!emit) (void)hipMemsetAsync(b.d_dtot.p, 0, b.regs.size() * DEPTH_TOTALS * 8, e->stream);
    hipLaunchKernelGGL(emit ? depth_runs_kernel<true> : depth_runs_kernel<false>, dim3((unsigned)b.n_tiles), dim3(TP), 0, e->stream,
                       b.p_regions, b.p_tile_region, b.d_depth.as<int32_t>(), e->n_targets > 0 ? b.d_targets.as<uint8_t>() : nullptr,
                       track_bounds(b.depth, e->depth_bins), b.depth.d_heads.as<int>(), b.depth.d_scan.as<int>(),
                       b.d_dtot.as<unsigned long long>(), b.depth.d_recs.as<DepthRun>(), (int)b.depth.cap);
}
void launch_ref_blocks(pa_encoder* e, bool emit) {
    pa_variant_batch& b = *e->variant;
    hipLaunchKernelGGL(emit ? ref_blocks_kernel<true> : ref_blocks_kernel<false>, dim3((unsigned)b.n_tiles), dim3(TP), 0, e->stream,
                       b.p_regions, b.p_tile_region, b.d_depth.as<int32_t>(), b.d_gq.as<uint8_t>(),
                       e->n_targets > 0 ? b.d_targets.as<uint8_t>() : nullptr, track_bounds(b.blocks, e->ref_bands),
                       b.blocks.d_heads.as<int>(), b.blocks.d_scan.as<int>(), b.blocks.d_recs.as<RefBlock>(), (int)b.blocks.cap);
}

// A track that is set: heads counted per tile, the counts scanned, the records emitted; the record count travels to the host
// before the run's one wait.  Room for the records: one per 16 rows and four more per tile -- a sixteenth of the worst case of
// a record per row (real coverage changes class a few times per kilobase) -- or the debug capacity the setting call read from
// the environment, or what an earlier run of the handle needed; a run with more heads than that is emitted a second time
// (finish_track).
int submit_track(pa_encoder* e, RunTrack& t, const pa_track_setting& set, const TrackSlots& slots, void (*launch)(pa_encoder*, bool)) {
    pa_variant_batch& b = *e->variant;
    hipStream_t st = e->stream;
    t.classes = set.n;
    const int64_t sized = set.cap > 0 ? set.cap : b.total_rows / 16 + 4 * (int64_t)b.n_tiles;
    t.cap = std::min<int64_t>(std::max(t.cap, sized), 0x7ffffff0);
    ENC_ALLOC(t.d_heads, (size_t)b.n_tiles * 4);             // (every tile writes its count: nothing to clear)
    ENC_ALLOC(t.d_scan, ((size_t)b.n_tiles + 1) * 4);
    ENC_ALLOC(t.d_recs, (size_t)t.cap * slots.rec_bytes);
    if (!t.h_count.ensure(8)) return pa::set_error(PA_ERR_HIP, "hipHostMalloc failed");
    ENC_HIP(hipEventRecord(e->ev[slots.ev], st));
    launch(e, false);
    hipLaunchKernelGGL(tile_offsets_kernel, dim3(1), dim3(1024), 0, st, t.d_heads.as<int>(), b.n_tiles, t.d_scan.as<int>());
    launch(e, true);
    ENC_HIP(hipEventRecord(e->ev[slots.ev + 1], st));
    ENC_HIP(hipGetLastError());
    ENC_HIP(hipMemcpyAsync(t.h_count.p, t.d_scan.as<int>() + b.n_tiles, sizeof(int), hipMemcpyDeviceToHost, st));
    return PA_OK;
}

// after the run's wait: the record count, and the second emit of a run whose records outgrew the buffer (every overflow is
// counted; the rows' values, the verdicts and the scanned offsets are where the first emit read them, so the records are exact)
int finish_track(pa_encoder* e, RunTrack& t, const TrackSlots& slots, void (*launch)(pa_encoder*, bool)) {
    t.calls += 1;
    t.n = *t.h_count.as<int>();
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e->ev[slots.ev], e->ev[slots.ev + 1]); e->variant->ms[slots.ms] = ms;     // the track's kernel x 2 + tile_offsets_kernel
    t.on = true;
    if (t.n <= t.cap) return PA_OK;
    t.on = false;                                  // (until the second emit is through)
    t.overflows += 1;
    t.cap = t.n;
    ENC_ALLOC(t.d_recs, (size_t)t.cap * slots.rec_bytes);
    launch(e, true);
    ENC_HIP(hipGetLastError());
    ENC_HIP(hipStreamSynchronize(e->stream));
    t.on = true;
    return PA_OK;
}

int submit_tracks(pa_encoder* e, const RunShape& w) {
    pa_variant_batch& b = *e->variant;
    if (e->depth_bins.n > 0) {
        const size_t tot_bytes = (size_t)w.n_regions * DEPTH_TOTALS * 8;
        ENC_ALLOC(b.d_dtot, tot_bytes);
        if (!b.h_dtot.ensure(tot_bytes)) return pa::set_error(PA_ERR_HIP, "hipHostMalloc failed");
        const int rc = submit_track(e, b.depth, e->depth_bins, DEPTH_SLOTS, launch_depth_runs);
        if (rc != PA_OK) return rc;
        ENC_HIP(hipMemcpyAsync(b.h_dtot.p, b.d_dtot.p, tot_bytes, hipMemcpyDeviceToHost, e->stream));
    }
    return e->ref_bands.n > 0 ? submit_track(e, b.blocks, e->ref_bands, BLOCK_SLOTS, launch_ref_blocks) : PA_OK;
}

int finish_tracks(pa_encoder* e) {
    pa_variant_batch& b = *e->variant;
    const int rc = e->depth_bins.n > 0 ? finish_track(e, b.depth, DEPTH_SLOTS, launch_depth_runs) : PA_OK;
    return rc == PA_OK && e->ref_bands.n > 0 ? finish_track(e, b.blocks, BLOCK_SLOTS, launch_ref_blocks) : rc;
}

// The records of the last run's track into the caller's columns (null: not wanted; `wanted`: one of them is not null): region,
// start and end for every track, `rest(k, record)` for the columns of this one.  what / noun: how the messages begin and what
// they call a record.
inline int32_t reported_class(int cls) { return cls == TRACK_OFF_TARGET ? -1 : cls; }

template <typename Rec, typename Rest>
int fetch_track(pa_encoder* e, const RunTrack& t, const char* what, const char* noun, bool wanted, int64_t capacity, int32_t* region,
                int64_t* start, int64_t* end, int64_t* n_out, Rest rest) {
    const pa_variant_batch& b = *e->variant;
    if (n_out) *n_out = t.n;
    if (!wanted) return PA_OK;
    if (capacity < t.n)
        return pa::set_error(PA_ERR_INVALID, std::string(what) + ": " + std::to_string(t.n) + " " + noun + ", room for " + std::to_string(capacity));
    if (t.n == 0) return PA_OK;
    ENC_HIP(hipSetDevice(e->device));
    std::vector<Rec> recs((size_t)t.n);
    ENC_HIP(hipMemcpyAsync(recs.data(), t.d_recs.p, recs.size() * sizeof(Rec), hipMemcpyDeviceToHost, e->stream));
    ENC_HIP(hipStreamSynchronize(e->stream));
    for (size_t k = 0; k < recs.size(); ++k) {
        const Rec& r = recs[k];
        if (r.region < 0 || r.region >= (int)b.regs.size() || (k > 0 && r.region < recs[k - 1].region))
            return pa::set_error(PA_ERR_HIP, std::string(what) + ": record " + std::to_string(k) + " names no region of the batch");
        const RegHost& rh = b.regs[(size_t)r.region];
        // a record ends where the next one of its region starts, the last one behind the window's last row
        const int64_t window_end = std::min<int64_t>(rh.L - 1, rh.q.candidate_region_end - rh.p.region_start) + 1;
        const int64_t stop = (k + 1 < recs.size() && recs[k + 1].region == r.region) ? recs[k + 1].row : window_end;
        if (region) region[k] = r.region;
        if (start) start[k] = rh.p.region_start + r.row;
        if (end) end[k] = rh.p.region_start + stop;
        rest(k, r);
    }
    return PA_OK;
}

int track_calls(pa_encoder* e, RunTrack pa_variant_batch::*track, int64_t* runs, int64_t* overflows) {
    if (!e) return pa::set_error(PA_ERR_INVALID, "null encoder");
    if (runs) *runs = e->variant ? (e->variant->*track).calls : 0;
    if (overflows) *overflows = e->variant ? (e->variant->*track).overflows : 0;
    return PA_OK;
}

// candidates and windows behind the counts, in the same submission: the votes grouped per site, the sites enumerated twice
// (counted, then written behind the scans of the tile totals), the windows gathered, the scans on their way to the host
int submit_candidates(pa_encoder* e, const RunShape& w) {
    pa_variant_batch& b = *e->variant;
    hipStream_t st = e->stream;
    ENC_ALLOC(b.d_rare_next, (size_t)b.ovf_cap * 4);
    ENC_ALLOC(b.d_cands, (size_t)b.cand_cap * sizeof(CandDesc));
    ENC_ALLOC(b.d_pos, (size_t)b.cand_cap * 8);
    ENC_ALLOC(b.d_depths, (size_t)b.cand_cap * 4);
    ENC_ALLOC(b.d_freqs, (size_t)b.cand_cap * 4);
    ENC_ALLOC(b.d_names, (size_t)b.cand_cap * 72);           // a name is a type character, at most 63 allele bytes and a NUL
    ENC_ALLOC(b.d_img32, (size_t)b.cand_cap * b.W * b.F * sizeof(int));
    ENC_ALLOC(b.d_img8, (size_t)b.cand_cap * b.W * b.F);
    CandArgs ca;
    ca.regions = b.p_regions; ca.rules = b.d_rules.as<pa_cand::Rule>(); ca.n_regions = w.n_regions; ca.n_tiles = b.n_tiles;
    ca.counters = w.counters; ca.region_counts = w.region_counts; ca.n_recs = b.d_tile_off.as<int>() + b.n_tiles;
    ca.rec_cap = b.rec_cap; ca.ovf_cap = b.ovf_cap; ca.pool_cap = b.pool_cap; ca.vote_cap = w.vote_cap;
    ca.sites = b.d_sites_dense.as<SiteRec>(); ca.votes = b.d_votes_dense.as<Vote>(); ca.grouped = b.d_grouped.as<Vote>();
    ca.ovf = b.d_ovf.as<int4>(); ca.rare_next = b.d_rare_next.as<int>();
    ca.ref = b.p_ref; ca.pool = b.d_pool.as<char>(); ca.pass = b.d_pass.as<uint8_t>();
    ca.row_slot = b.d_row_slot.as<int>(); ca.aux = b.d_aux.as<SiteAux>(); ca.large = b.d_large.as<int>();
    ca.cinfo = b.d_czero.as<int>(); ca.tile_nc = ca.cinfo + CI_N; ca.tile_nb = ca.tile_nc + b.n_tiles;
    ca.tile_c0 = b.d_cscan.as<int>(); ca.tile_b0 = ca.tile_c0 + b.n_tiles + 1;
    ca.cand_cap = b.cand_cap; ca.mid = b.mid;
    ca.cands = b.d_cands.as<CandDesc>(); ca.positions = b.d_pos.as<int64_t>(); ca.depths = b.d_depths.as<int32_t>();
    ca.freqs = b.d_freqs.as<int32_t>(); ca.names = b.d_names.as<char>();
    const dim3 g_small((unsigned)std::min<int64_t>(b.total_rows, 8192)), g_large((unsigned)std::min<int64_t>(b.total_rows, 1536));
    ENC_HIP(hipMemsetAsync(b.d_czero.p, 0, w.n_czero * 4, st));
    hipLaunchKernelGGL(group_votes_kernel, dim3((unsigned)w.n_regions), dim3(1024), 0, st, ca);
    hipLaunchKernelGGL((enumerate_sites_kernel<64, false>), g_small, dim3(64), 0, st, ca);
    hipLaunchKernelGGL((enumerate_sites_kernel<CAND_SITE_MAX, false>), g_large, dim3(64), 0, st, ca);
    hipLaunchKernelGGL(tile_offsets_kernel, dim3(1), dim3(1024), 0, st, ca.tile_nc, b.n_tiles, b.d_cscan.as<int>());
    hipLaunchKernelGGL(tile_offsets_kernel, dim3(1), dim3(1024), 0, st, ca.tile_nb, b.n_tiles, b.d_cscan.as<int>() + b.n_tiles + 1);
    hipLaunchKernelGGL((enumerate_sites_kernel<64, true>), g_small, dim3(64), 0, st, ca);
    hipLaunchKernelGGL((enumerate_sites_kernel<CAND_SITE_MAX, true>), g_large, dim3(64), 0, st, ca);
    ENC_HIP(hipEventRecord(e->ev[4], st));
    hipLaunchKernelGGL(gather_windows_n_kernel, dim3((unsigned)std::min(b.cand_cap, 16384)), dim3(64), 0, st, ca, b.d_mat.as<int>(),
                       b.W, b.F, b.d_img32.as<int>(), b.d_img8.as<int8_t>());
    ENC_HIP(hipEventRecord(e->ev[5], st));
    ENC_HIP(hipGetLastError());
    ENC_HIP(hipMemcpyAsync(b.h_cscan.p, b.d_cscan.p, w.n_cscan * 4, hipMemcpyDeviceToHost, st));
    ENC_HIP(hipMemcpyAsync(b.h_cscan.as<int>() + w.n_cscan, b.d_czero.p, CI_N * 4, hipMemcpyDeviceToHost, st));
    return PA_OK;
}

// what the device reported about the input: unpack_clip_kernel while the batch was staged (the copy is long done; with it the
// reads per region and the sample's counts), then the counters of the run
int check_reports(pa_encoder* e, const RunShape& w) {
    pa_variant_batch& b = *e->variant;
    const int n_regions = w.n_regions;
    if (b.packed) {
        pa_enc::sample_collect(e);
        const int* hl = b.h_live.as<int>();
        if (hl[n_regions] > 0)
            return pa::set_error(PA_ERR_INVALID, "packed read " + std::to_string(hl[n_regions] - 1) + ": its CIGAR walks over more bases than the record holds");
        if (hl[n_regions + 1] > 0)
            return pa::set_error(PA_ERR_UNSUPPORTED, "packed read " + std::to_string(hl[n_regions + 1] - 1) +
                                                         ": a CIGAR operation of 2^24 bases or more (take the host-clipped form for this batch)");
        for (int r = 0; r < n_regions; ++r) b.live[(size_t)r] = hl[r];
    }
    if (w.host_counters[CT_ERR] > 0) {
        const int64_t g = w.host_counters[CT_ERR] - 1;
        size_t r = 0;
        while (r + 1 < b.regs.size() && b.regs[r + 1].read_base <= g) ++r;
        return pa::set_error(PA_ERR_INVALID, "CIGAR of read " + std::to_string(g - b.regs[r].read_base) + (n_regions > 1 ? " of region " + std::to_string(r) : "") +
                                                 " runs past its sequence");
    }
    if (w.host_counters[CT_VOTES] > w.vote_cap) return pa::set_error(PA_ERR_INVALID, "more indel votes than CIGAR operations (corrupt pileup)");
    return PA_OK;
}

// the kernels enumerated this run: nothing left for the host -- the counts per region are differences of the tile offsets
int take_device_results(pa_encoder* e, const RunShape& w, int64_t* n_candidates) {
    pa_variant_batch& b = *e->variant;
    const int* c0 = b.h_cscan.as<int>();
    int tile = 0;
    for (int r = 0; r < w.n_regions; ++r) {
        const int nt = (b.regs[(size_t)r].L + 1 + TP - 1) / TP;
        b.region_n[(size_t)r] = c0[tile + nt] - c0[tile];
        tile += nt;
    }
    b.n = c0[b.n_tiles];
    b.name_bytes = c0[w.n_cscan - 1];
    b.dev_results = true;
    b.dev_lists = true;
    b.dev_calls += 1;
    if (n_candidates)
        for (int r = 0; r < w.n_regions; ++r) n_candidates[r] = b.region_n[(size_t)r];
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e->ev[3], e->ev[4]); b.ms[12] = ms;  // group_votes_kernel ... enumerate_sites_kernel (both forms)
    (void)hipEventElapsedTime(&ms, e->ev[4], e->ev[5]); b.ms[3] = ms;   // gather_windows_n_kernel
    return PA_OK;
}

// the host's enumeration: the dense lists downloaded, sorted and enumerated region by region on the pool, the candidates sent
// back and their windows gathered
int enumerate_on_host(pa_encoder* e, const RunShape& w, int64_t* n_candidates) {
    pa_variant_batch& b = *e->variant;
    hipStream_t st = e->stream;
    const int n_regions = w.n_regions;
    const int* host_rc = w.host_counters + CT_N;
    if (w.dev) b.host_calls += 1;     // refused by the kernels (CI_REFUSED): enumerated here, as with the switch off
    // region r's sites / votes are [s0[r], s0[r + 1]) / [v0[r], v0[r + 1]) of the dense lists
    std::vector<size_t> s0((size_t)n_regions + 1, 0), v0((size_t)n_regions + 1, 0), o0((size_t)n_regions + 1, 0);
    for (int r = 0; r < n_regions; ++r) {
        s0[(size_t)r + 1] = s0[(size_t)r] + (size_t)host_rc[2 * r];
        v0[(size_t)r + 1] = v0[(size_t)r] + (size_t)host_rc[2 * r + 1];
    }
    const size_t n_sites = s0[(size_t)n_regions], n_votes = v0[(size_t)n_regions];
    const int n_ovf = w.host_counters[CT_OVF], n_pool = w.host_counters[CT_POOL];
    float ms = 0;
    if (!b.h_sites.ensure(n_sites * sizeof(SiteRec) + 64) || !b.h_votes.ensure(n_votes * sizeof(Vote) + 64) ||
        !b.h_pool.ensure((size_t)n_pool * POOL_SLOT + 64))
        return pa::set_error(PA_ERR_HIP, "hipHostMalloc failed");
    const char* pool = b.h_pool.as<char>();
    SiteRec* sites = b.h_sites.as<SiteRec>();
    Vote* votes = b.h_votes.as<Vote>();
    std::vector<int4> ovf((size_t)n_ovf);
    if (n_sites) ENC_HIP(hipMemcpyAsync(sites, b.d_sites_dense.p, n_sites * sizeof(SiteRec), hipMemcpyDeviceToHost, st));
    if (n_votes) ENC_HIP(hipMemcpyAsync(votes, b.d_votes_dense.p, n_votes * sizeof(Vote), hipMemcpyDeviceToHost, st));
    if (n_ovf) ENC_HIP(hipMemcpyAsync(ovf.data(), b.d_ovf.p, ovf.size() * sizeof(int4), hipMemcpyDeviceToHost, st));
    if (n_pool) ENC_HIP(hipMemcpyAsync(b.h_pool.p, b.d_pool.p, (size_t)n_pool * POOL_SLOT, hipMemcpyDeviceToHost, st));
    ENC_HIP(hipStreamSynchronize(st));
    const auto t_host = std::chrono::steady_clock::now();
    if (n_ovf) {                                                 // rare alphabet: a handful per batch, grouped here
        std::sort(ovf.begin(), ovf.end(), [](const int4& x, const int4& y) { return x.w < y.w; });
        for (const int4& o : ovf) o0[(size_t)o.w + 1] += 1;
    }
    for (int r = 0; r < n_regions; ++r) o0[(size_t)r + 1] += o0[(size_t)r];
    b.ms[6] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host).count();
    std::vector<RegionOut> outs((size_t)n_regions);
    const std::function<void(int)> work = [&](int r) {
        std::sort(sites + s0[(size_t)r], sites + s0[(size_t)r + 1], [](const SiteRec& x, const SiteRec& y) { return x.idx < y.idx; });
        // votes by (site, type, allele): one 64-bit key per vote decides nearly every comparison (28 bits of site, 2 of type, the
        // first 34 bits of the allele); the rare ties fall back to the full order
        const AlleleSrc pile{b.regs[(size_t)r].p.reference, pool};
        Vote* vb = votes + v0[(size_t)r];
        const size_t nv = v0[(size_t)r + 1] - v0[(size_t)r];
        std::vector<std::pair<uint64_t, uint32_t>> order(nv);
        for (size_t k = 0; k < nv; ++k)
            order[k] = {((uint64_t)vb[k].idx << 36) | ((uint64_t)(vb[k].meta & 3u) << 34) | (vb[k].prefix >> 30), (uint32_t)k};
        std::sort(order.begin(), order.end(), [&](const std::pair<uint64_t, uint32_t>& x, const std::pair<uint64_t, uint32_t>& y) {
            return x.first != y.first ? x.first < y.first : vote_less(vb[x.second], vb[y.second], pile);
        });
        std::vector<Vote> sorted(nv);
        for (size_t k = 0; k < nv; ++k) sorted[k] = vb[order[k].second];
        std::copy(sorted.begin(), sorted.end(), vb);
        enumerate_region(b.regs[(size_t)r], r, b.mid, sites + s0[(size_t)r], s0[(size_t)r + 1] - s0[(size_t)r], votes + v0[(size_t)r],
                         v0[(size_t)r + 1] - v0[(size_t)r], ovf.data() + o0[(size_t)r], o0[(size_t)r + 1] - o0[(size_t)r], pool, outs[(size_t)r]);
    };
    if (n_regions < 4 || b.host_threads == 1) {
        for (int r = 0; r < n_regions; ++r) work(r);
    } else {
        if (!b.pool) {
            const char* env = getenv("PA_ENCODER_HOST_THREADS");
            // a burst of ~0.3 ms tasks, one per region: a quarter of the hardware threads even where a cgroup quota grants fewer
            // CPUs on average (the quota is per 100 ms period; measured on the 16-of-256 box: 16 threads 1.45 ms per 64 regions,
            // 32 threads 0.94 ms)
            const int dflt = b.host_threads > 0 ? b.host_threads : std::max(usable_cpus(), (int)std::thread::hardware_concurrency() / 4);
            b.pool.reset(new RegionPool(std::max(1, std::min(env ? atoi(env) : dflt, 64)) - 1));
        }
        b.pool->run(n_regions, work);
    }
    b.ms[7] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host).count();   // ... + the regions' threads
    std::vector<CandDesc> cands;
    for (int r = 0; r < n_regions; ++r) {
        const RegionOut& o = outs[(size_t)r];
        b.region_n[(size_t)r] = (int64_t)o.cands.size();
        cands.insert(cands.end(), o.cands.begin(), o.cands.end());
        b.positions.insert(b.positions.end(), o.positions.begin(), o.positions.end());
        b.depths.insert(b.depths.end(), o.depths.begin(), o.depths.end());
        b.freqs.insert(b.freqs.end(), o.freqs.begin(), o.freqs.end());
        b.names += o.names;
    }
    b.ms[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host).count();   // host enumeration
    b.n = (int64_t)cands.size();
    if (n_candidates)
        for (int r = 0; r < n_regions; ++r) n_candidates[r] = b.region_n[(size_t)r];
    if (b.n > 0) {
        ENC_ALLOC(b.d_cands, cands.size() * sizeof(CandDesc));
        ENC_ALLOC(b.d_img32, (size_t)b.n * b.W * b.F * sizeof(int));
        ENC_ALLOC(b.d_img8, (size_t)b.n * b.W * b.F);
        ENC_HIP(hipMemcpyAsync(b.d_cands.p, cands.data(), cands.size() * sizeof(CandDesc), hipMemcpyHostToDevice, st));
        ENC_HIP(hipEventRecord(e->ev[4], st));
        hipLaunchKernelGGL(gather_windows_kernel, dim3((unsigned)b.n), dim3(64), 0, st, b.d_mat.as<int>(), b.p_regions,
                           b.d_cands.as<CandDesc>(), b.W, b.F, b.mid, b.d_img32.as<int>(), b.d_img8.as<int8_t>());
        ENC_HIP(hipEventRecord(e->ev[5], st));
        ENC_HIP(hipGetLastError());
        ENC_HIP(hipStreamSynchronize(st));
        (void)hipEventElapsedTime(&ms, e->ev[4], e->ev[5]); b.ms[3] = ms;   // gather_windows_kernel
    }
    return PA_OK;
}

int run_staged(pa_encoder* e, int64_t* n_candidates) {
    if (!e || !e->variant || !e->variant->staged) return pa::set_error(PA_ERR_INVALID, "no staged batch");
    ENC_HIP(hipSetDevice(e->device));
    pa_variant_batch& b = *e->variant;
    hipStream_t st = e->stream;
    const int n_regions = (int)b.regs.size();
    b.n = 0;
    b.region_n.assign((size_t)n_regions, 0);
    b.positions.clear(); b.depths.clear(); b.freqs.clear(); b.names.clear();
    b.dev_results = b.dev_lists = false;
    for (RunTrack* t : {&b.depth, &b.blocks}) { t->on = false; t->n = 0; }
    for (int k = 0; k < 8; ++k) b.ms[k] = 0;          // ([8], [9] belong to the staging of this batch)
    if (n_regions == 0) {
        b.depth.on = (b.depth.classes = e->depth_bins.n) > 0;       // (no region: no record, no total)
        b.blocks.on = (b.blocks.classes = e->ref_bands.n) > 0;
        return PA_OK;
    }
    const auto t_begin = std::chrono::steady_clock::now();
    RunShape w;
    int rc = size_workspaces(e, w);
    if (rc != PA_OK) return rc;
    if (b.packed && !b.sampled) {     // deep intervals sampled down before anything reads the pairs (once per staged batch)
        std::vector<int32_t> region_pairs((size_t)n_regions + 1);
        for (int r = 0; r < n_regions; ++r) region_pairs[(size_t)r] = (int32_t)b.regs[(size_t)r].read_base;
        region_pairs[(size_t)n_regions] = (int32_t)b.total_reads;
        rc = pa_enc::sample_pairs(e, n_regions, region_pairs.data(), b.d_reads.as<ReadRec>(), b.d_live.as<int>(), b.h_live.as<int>());
        if (rc != PA_OK) return rc;
        b.sampled = true;
    }
    b.dev_results = false;
    b.dev_lists = false;
    b.ms[12] = 0;
    b.ms[13] = 0;
    b.ms[14] = 0;
    if (w.dev) ENC_HIP(hipMemcpyAsync(b.d_rules.p, b.h_rules.p, (size_t)n_regions * sizeof(pa_cand::Rule), hipMemcpyHostToDevice, st));
    int* host_counters = w.host_counters;
    bool on_device = false;           // this call's candidates were enumerated by the kernels
    for (int attempt = 0;; ++attempt) {       // one submission and one wait each; repeated with room when a buffer was too small
        rc = submit_counts(e, w);
        if (rc == PA_OK && w.dev) rc = submit_candidates(e, w);
        if (rc == PA_OK) rc = submit_tracks(e, w);
        if (rc != PA_OK) return rc;
        ENC_HIP(hipMemcpyAsync(host_counters, w.counters, ((size_t)CT_N + 2 * (size_t)n_regions) * 4, hipMemcpyDeviceToHost, st));
        ENC_HIP(hipMemcpyAsync(host_counters + CT_N + 2 * n_regions, b.d_tile_off.as<int>() + b.n_tiles, sizeof(int), hipMemcpyDeviceToHost, st));
        ENC_HIP(hipStreamSynchronize(st));
        const int n_recs = host_counters[CT_N + 2 * n_regions];
        if (n_recs > b.rec_cap || host_counters[CT_OVF] > b.ovf_cap || host_counters[CT_POOL] > b.pool_cap) {
            if (attempt >= 2) return pa::set_error(PA_ERR_HIP, "encoder record buffers could not be sized");
            b.rec_cap = std::max(b.rec_cap, n_recs + 1024);
            b.ovf_cap = std::max(b.ovf_cap, host_counters[CT_OVF] + 1024);
            b.pool_cap = std::max(b.pool_cap, host_counters[CT_POOL] + 1024);
            continue;
        }
        if (w.dev && host_counters[CT_ERR] <= 0 && host_counters[CT_VOTES] <= w.vote_cap && b.h_cscan.as<int>()[w.n_cscan + CI_REFUSED] == 0) {
            const int found = b.h_cscan.as<int>()[b.n_tiles];
            if (found > b.cand_cap) {                            // more candidates than the buffers hold: nothing was written
                if (attempt >= 3) return pa::set_error(PA_ERR_HIP, "encoder candidate buffers could not be sized");
                b.cand_cap = (int)std::min<int64_t>(0x7ffffff0, (int64_t)found + found / 4 + 1024);
                continue;
            }
            on_device = true;
        }
        break;
    }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e->ev[0], e->ev[1]); b.ms[0] = ms;       // records: count pass + offsets + fill pass
    (void)hipEventElapsedTime(&ms, e->ev[1], e->ev[2]); b.ms[1] = ms;       // tile_count_kernel
    (void)hipEventElapsedTime(&ms, e->ev[2], e->ev[3]); b.ms[2] = ms;       // compact_votes_kernel + pack_results_kernel
    if (b.packed && b.ms[8] == 0 && b.ms[9] == 0) {
        (void)hipEventElapsedTime(&ms, e->ev[6], e->ev[7]); b.ms[8] = ms;   // upload of the arena and the tables
        (void)hipEventElapsedTime(&ms, e->ev[7], e->ev[8]); b.ms[9] = ms;   // unpack_clip_kernel
    }
    rc = check_reports(e, w);
    if (rc == PA_OK) rc = finish_tracks(e);
    if (rc == PA_OK) rc = on_device ? take_device_results(e, w, n_candidates) : enumerate_on_host(e, w, n_candidates);
    if (rc != PA_OK) return rc;
    b.ms[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();  // whole run, host clock
    return PA_OK;
}

}  // namespace

int pa_enc::sample_pairs(pa_encoder* e, int32_t n_regions, const int32_t* region_pairs, ReadRec* d_reads, int* d_live, int* h_live) {
    pa_sampler& s = e->sampler;
    s.pending = 0;
    if (!s.on || n_regions <= 0) return PA_OK;
    // an interval can need the sample when rate * n < n for some n it may have, or when it has more pairs than the cap
    std::vector<SampRec> tab;
    for (int r = 0; r < n_regions; ++r) {
        const int32_t pairs = region_pairs[r + 1] - region_pairs[r];
        if (pairs > 0 && (s.rate < 1.0 || pairs > s.cap)) tab.push_back(SampRec{r, region_pairs[r], region_pairs[r + 1], 0});
    }
    if (tab.empty()) return PA_OK;
    const size_t c = tab.size(), o_out = c * sizeof(SampRec), bytes = o_out + c * sizeof(int2);
    if (!s.h_tab.ensure(bytes)) return pa::set_error(PA_ERR_HIP, "hipHostMalloc failed");
    ENC_ALLOC(s.d_tab, bytes);
    ENC_ALLOC(s.d_keep, (size_t)region_pairs[n_regions] + 64);
    std::memcpy(s.h_tab.p, tab.data(), o_out);
    hipStream_t st = e->stream;
    char* dt = s.d_tab.as<char>();
    ENC_HIP(hipMemcpyAsync(dt, s.h_tab.p, o_out, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(reservoir_keep_kernel, dim3((unsigned)c), dim3(RS_T), 0, st, reinterpret_cast<const SampRec*>(dt), d_reads, d_live,
                       s.d_keep.as<uint8_t>(), reinterpret_cast<int2*>(dt + o_out), s.seed, (int)s.cap, s.rate);
    ENC_HIP(hipGetLastError());
    ENC_HIP(hipMemcpyAsync(s.h_tab.as<char>() + o_out, dt + o_out, c * sizeof(int2), hipMemcpyDeviceToHost, st));
    ENC_HIP(hipMemcpyAsync(h_live, d_live, ((size_t)n_regions + 2) * 4, hipMemcpyDeviceToHost, st));
    s.pending = (int)c;
    return PA_OK;
}

int pa_enc::selection_view(pa_encoder* e, int device, hipStream_t stream, SelectionView* out) {
    if (!e || !out) return pa::set_error(PA_ERR_INVALID, "null argument");
    if (!e->variant || !e->variant->staged) return pa::set_error(PA_ERR_INVALID, "select candidates: the encoder has no variant run");
    if (e->device != device) return pa::set_error(PA_ERR_INVALID, "select candidates: the encoder and the selector are on different devices");
    pa_variant_batch& b = *e->variant;
    const size_t n = (size_t)b.n;
    if (!b.dev_lists) {               // enumerated on the host: its lists go where the device enumeration would have left them
        if (b.positions.size() != n || b.depths.size() != n || b.freqs.size() != n)
            return pa::set_error(PA_ERR_INVALID, "select candidates: the last run left no lists");
        b.name_bytes = (int64_t)b.names.size();
        ENC_ALLOC(b.d_pos, n * 8 + 8);
        ENC_ALLOC(b.d_depths, n * 4 + 8);
        ENC_ALLOC(b.d_freqs, n * 4 + 8);
        ENC_ALLOC(b.d_names, b.names.size() + 8);
        if (n) {
            ENC_HIP(hipMemcpyAsync(b.d_pos.p, b.positions.data(), n * 8, hipMemcpyHostToDevice, stream));
            ENC_HIP(hipMemcpyAsync(b.d_depths.p, b.depths.data(), n * 4, hipMemcpyHostToDevice, stream));
            ENC_HIP(hipMemcpyAsync(b.d_freqs.p, b.freqs.data(), n * 4, hipMemcpyHostToDevice, stream));
            ENC_HIP(hipMemcpyAsync(b.d_names.p, b.names.data(), b.names.size(), hipMemcpyHostToDevice, stream));
        }
        b.dev_lists = true;
    }
    out->n = b.n;
    out->name_bytes = b.name_bytes;
    out->positions = b.d_pos.as<int64_t>();
    out->depths = b.d_depths.as<int32_t>();
    out->supports = b.d_freqs.as<int32_t>();
    out->names = b.d_names.as<char>();
    out->regions.clear();
    int64_t first = 0, ref_off = 0;
    for (size_t r = 0; r < b.regs.size(); ++r) {
        const pa_pileup& p = b.regs[r].p;
        out->regions.push_back(SelectionRegion{first, p.region_start, p.reference_len, b.p_ref + ref_off});
        first += r < b.region_n.size() ? b.region_n[r] : 0;
        ref_off += p.reference_len;
    }
    return PA_OK;
}

void pa_enc::sample_collect(pa_encoder* e) {
    pa_sampler& s = e->sampler;
    const int2* out = reinterpret_cast<const int2*>(s.h_tab.as<char>() + (size_t)s.pending * sizeof(SampRec));
    for (int k = 0; k < s.pending; ++k)
        if (out[k].y < out[k].x) {
            s.regions += 1;
            s.dropped += out[k].x - out[k].y;
        }
    s.pending = 0;
}

// The packed reads of a batch of regions clipped and decoded on the device WITHOUT the variant encoder's tables: what the polish
// image chain (encoder_polish.hip) starts from.  Same arena / read / pair tables as stage_packed, same block, same pair walk (with
// the room a region can fill) and the same submission; the regions are given by their bounds alone.  Nothing here waits for
// the device.
int pa_enc::unpack_packed_regions(pa_encoder* e, int32_t n_regions, const int64_t* region_start, const int64_t* region_end,
                                  const uint8_t* arena, int64_t arena_bytes, const pa_packed_read* reads, int32_t n_reads,
                                  const int32_t* pair_read, const int32_t* region_pairs, int32_t extra_ops_per_pair, UnpackedReads* out) {
    const std::vector<int64_t> soff = take_seq_offsets(e);
    if (!soff.empty() && (int64_t)soff.size() != n_reads)
        return pa::set_error(PA_ERR_INVALID, "the base offsets set for this call are not one per packed read");
    if (!e || !out || n_regions < 0 || (n_regions > 0 && (!region_start || !region_end || !region_pairs)) || arena_bytes < 0 || n_reads < 0 ||
        (n_reads > 0 && (!reads || !pair_read)))
        return pa::set_error(PA_ERR_INVALID, "null argument");
    ENC_HIP(hipSetDevice(e->device));
    if (!e->variant) e->variant = new pa_variant_batch();
    pa_variant_batch& b = *e->variant;
    int rc = check_resident(b, arena, n_reads, arena_bytes);
    if (rc != PA_OK) return rc;
    b.staged = false;               // (the variant encoder's staged batch, if any, shares these buffers)
    const int64_t n_pairs = n_regions ? region_pairs[n_regions] : 0;
    if (n_pairs < 0 || (n_regions && region_pairs[0] != 0)) return pa::set_error(PA_ERR_INVALID, "region_pairs must start at 0 and ascend");
    const PackedBlock L = lay_out_block(n_regions, 0, (size_t)n_reads * sizeof(PackedRead), (size_t)n_pairs * sizeof(PairRec), soff.size() * 8, 0);
    if (!b.h_meta.ensure(L.bytes) || !b.h_live.ensure(((size_t)n_regions + 2) * 4)) return pa::set_error(PA_ERR_HIP, "hipHostMalloc failed");
    ENC_ALLOC(b.d_meta, L.bytes);
    char* hm = b.h_meta.as<char>();
    RegRec* regrecs = reinterpret_cast<RegRec*>(hm + L.o_reg);
    int64_t* rstart = reinterpret_cast<int64_t*>(hm + L.o_start);
    RegionSums sums;
    for (int r = 0; r < n_regions; ++r) {
        pa_pileup p{};
        p.region_start = rstart[r] = region_start[r];
        p.region_end = region_end[r];
        rc = region_pass(p, nullptr, nullptr, 0, 0, 0, sums, nullptr, regrecs[r]);
        if (rc != PA_OK) return rc;
        if (region_pairs[r + 1] < region_pairs[r]) return pa::set_error(PA_ERR_INVALID, "region_pairs must ascend");
    }
    if (n_reads) std::memcpy(hm + L.o_reads, reads, (size_t)n_reads * sizeof(PackedRead));
    if (!soff.empty()) std::memcpy(hm + L.o_soff, soff.data(), soff.size() * 8);
    std::vector<int64_t> seq_base((size_t)n_regions + 1);
    std::vector<int32_t> op_base((size_t)n_regions + 1);
    rc = walk_pairs(n_regions, region_pairs, pair_read, reads, n_reads, soff, arena_bytes, regrecs, reinterpret_cast<PairRec*>(hm + L.o_pairs),
                    seq_base.data(), op_base.data());
    if (rc != PA_OK) return rc;
    const int64_t total_bases = seq_base[(size_t)n_regions], total_ops = op_base[(size_t)n_regions];
    const int64_t extra_ops = extra_ops_per_pair < 0 ? 0 : total_bases + n_pairs * (int64_t)extra_ops_per_pair;
    if (total_ops + extra_ops > 0x7ffffff0) return pa::set_error(PA_ERR_INVALID, BATCH_TOO_LARGE);
    rc = submit_unpack(e, n_regions, n_pairs, arena, arena_bytes, n_reads, L, block_tables(b, L, !soff.empty()), total_bases, total_ops, extra_ops);
    if (rc != PA_OK) return rc;
    out->reads = b.d_reads.as<ReadRec>(); out->cigar_op = b.d_cig_op.as<int32_t>(); out->cigar_len = b.d_cig_len.as<int32_t>();
    out->seq = b.d_seq.as<char>(); out->d_live = b.d_live.as<int>(); out->h_live = b.h_live.as<int>();
    out->n_pairs = n_pairs; out->total_bases = total_bases; out->total_ops = total_ops; out->extra_ops = extra_ops;
    return PA_OK;
}

#ifdef PA_ENC_STAMP
extern "C" int pa_encoder_debug_cycles(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_enc_cycles), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    if (reset) {
        unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_enc_cycles), zero, sizeof zero) != hipSuccess) return -1;
    }
    return 0;
}
#endif

extern "C" {

int pa_encoder_create(int32_t device, void* hip_stream, pa_encoder** out) {
    if (!out) return pa::set_error(PA_ERR_INVALID, "null argument");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return pa::set_error(PA_ERR_NO_DEVICE, "no HIP device visible: the pepper_amd encoder has no CPU fallback");
    if (device < 0 || device >= count) return pa::set_error(PA_ERR_INVALID, "device ordinal out of range");
    ENC_HIP(hipSetDevice(device));
    // PEPPER_AMD_BLOCKING_SYNC=1: waits on the device sleep instead of spinning (sixteen image-generation workers spinning in
    // hipStreamSynchronize use up the CPUs the other workers' host stages need); refused once the device is in use: ignored
    if (const char* v = getenv("PEPPER_AMD_BLOCKING_SYNC"))
        if (v[0] == '1') (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
    auto* e = new pa_encoder();
    e->device = device;
    if (hip_stream) e->stream = static_cast<hipStream_t>(hip_stream);
    else {
        if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) {
            delete e;
            return pa::set_error(PA_ERR_HIP, "hipStreamCreate failed");
        }
        e->own_stream = true;
    }
    for (hipEvent_t& ev : e->ev)
        if (hipEventCreate(&ev) != hipSuccess) {
            pa_encoder_destroy(e);
            return pa::set_error(PA_ERR_HIP, "hipEventCreate failed");
        }
    *out = e;
    return PA_OK;
}

void pa_encoder_destroy(pa_encoder* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (hipEvent_t ev : e->ev)
        if (ev) (void)hipEventDestroy(ev);
    pa_variant_batch_free(e->variant);
    pa_polish_batch_free(e->polish);
    if (e->realigner) pa_realigner_destroy(e->realigner);      // (the image chain's, on this encoder's stream)
    if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

int pa_encoder_stage_batch(pa_encoder* e, int32_t n_regions, const pa_pileup* pileups, const pa_summary_params* params) {
    return stage_batch(e, n_regions, pileups, params);
}

int pa_encoder_run_staged(pa_encoder* e, int64_t* n_candidates) { return run_staged(e, n_candidates); }

void* pa_encoder_host_arena(pa_encoder* e, int64_t bytes) {
    if (!e || bytes < 0 || hipSetDevice(e->device) != hipSuccess) return nullptr;
    if (!e->variant) e->variant = new pa_variant_batch();
    if (e->stream) (void)hipStreamSynchronize(e->stream);        // (an upload out of the old block may still be running)
    return e->variant->h_arena.ensure((size_t)bytes) ? e->variant->h_arena.p : nullptr;
}

void* pa_encoder_host_span(pa_encoder* e, int64_t bytes) {
    if (!e || bytes < 0 || hipSetDevice(e->device) != hipSuccess) return nullptr;
    if (!e->variant) e->variant = new pa_variant_batch();
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    return e->variant->h_comp.ensure((size_t)bytes) ? e->variant->h_comp.p : nullptr;
}

// BGZF members -> the encoder's device arena (inflate.hip: one wavefront per member), and a copy for the host's record walk
int pa_encoder_inflate_bgzf(pa_encoder* e, const uint8_t* comp, int64_t comp_bytes, int32_t n_blocks, const int64_t* comp_off,
                            const int32_t* comp_len, const int64_t* out_off, const int32_t* out_len, int64_t out_bytes,
                            uint8_t* host_out) {
    if (!e || n_blocks < 0 || comp_bytes < 0 || out_bytes < 0 ||
        (n_blocks > 0 && (!comp || !comp_off || !comp_len || !out_off || !out_len)))
        return pa::set_error(PA_ERR_INVALID, "null or negative argument");
    for (int32_t k = 0; k < n_blocks; ++k)
        if (comp_off[k] < 0 || comp_len[k] < 0 || comp_off[k] + comp_len[k] > comp_bytes || out_off[k] < 0 || out_len[k] < 0 ||
            out_off[k] + out_len[k] > out_bytes)
            return pa::set_error(PA_ERR_INVALID, "BGZF block " + std::to_string(k) + " lies outside the buffers");
    ENC_HIP(hipSetDevice(e->device));
    if (!e->variant) e->variant = new pa_variant_batch();
    pa_variant_batch& b = *e->variant;
    b.resident_bytes = 0;
    b.walk.valid = b.pk.valid = false;            // (headers and tables describe the span that was resident)
    b.ms[10] = b.ms[11] = 0;
    if (n_blocks == 0) return PA_OK;
    hipStream_t st = e->stream;
    const size_t nb = (size_t)n_blocks, table_bytes = nb * 28;
    ENC_ALLOC(b.d_arena, (size_t)out_bytes + 256);
    ENC_ALLOC(b.d_comp, (size_t)comp_bytes + 64);
    ENC_ALLOC(b.d_inf, table_bytes);
    if (!b.h_inf.ensure(table_bytes)) return pa::set_error(PA_ERR_HIP, "hipHostMalloc failed in the inflate tables");
    char* hm = b.h_inf.as<char>();
    std::memcpy(hm, comp_off, nb * 8);
    std::memcpy(hm + nb * 8, out_off, nb * 8);
    std::memcpy(hm + nb * 16, comp_len, nb * 4);
    std::memcpy(hm + nb * 20, out_len, nb * 4);
    // The tables are read, and the status words written, in the page-locked block itself (it is mapped into the device's
    // address space): each of a job's small copies otherwise waits for CUs behind other workers' long-lived inflate
    // wavefronts (the runtime's copy kernels: ~1.5 ms apiece in the trace of DESIGN.md 4.4).
    void* mapped = nullptr;
    if (hipHostGetDevicePointer(&mapped, hm, 0) != hipSuccess || !mapped) mapped = nullptr;
    std::memset(hm + nb * 24, 0xff, nb * 4);                  // (a member the kernel never reaches reads as an error)
    char* dm = mapped ? static_cast<char*>(mapped) : b.d_inf.as<char>();
    const auto t0 = std::chrono::steady_clock::now();
    ENC_HIP(hipMemcpyAsync(b.d_comp.p, comp, (size_t)comp_bytes, hipMemcpyHostToDevice, st));
    if (!mapped) ENC_HIP(hipMemcpyAsync(dm, hm, nb * 24, hipMemcpyHostToDevice, st));
    ENC_HIP(hipEventRecord(e->ev[10], st));
    pa::launch_bgzf_inflate(st, b.d_comp.as<uint8_t>(), reinterpret_cast<const int64_t*>(dm), reinterpret_cast<const int32_t*>(dm + nb * 16),
                            reinterpret_cast<const int64_t*>(dm + nb * 8), reinterpret_cast<const int32_t*>(dm + nb * 20),
                            b.d_arena.as<uint8_t>(), reinterpret_cast<int32_t*>(dm + nb * 24), n_blocks, comp_bytes);
    ENC_HIP(hipGetLastError());
    ENC_HIP(hipEventRecord(e->ev[11], st));
    if (!mapped) ENC_HIP(hipMemcpyAsync(hm + nb * 24, dm + nb * 24, nb * 4, hipMemcpyDeviceToHost, st));
    if (host_out && out_bytes > 0) ENC_HIP(hipMemcpyAsync(host_out, b.d_arena.p, (size_t)out_bytes, hipMemcpyDeviceToHost, st));
    ENC_HIP(hipStreamSynchronize(st));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, e->ev[10], e->ev[11]) == hipSuccess) b.ms[10] = ms;
    b.ms[11] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const int32_t* status = reinterpret_cast<const int32_t*>(hm + nb * 24);
    for (int32_t k = 0; k < n_blocks; ++k)
        if (status[k] != 0)
            return pa::set_error(PA_ERR_INVALID, "BGZF block " + std::to_string(k) + ": " + pa::inflate_status_text(status[k]));
    b.resident_bytes = out_bytes;
    return PA_OK;
}

// The record headers of the span pa_encoder_inflate_bgzf left on the device (inflate.hip: record_chase_kernel and friends):
// everything up to the wait -- the walk's launches and, where the page-locked block is not mapped, the copies of its tail words
static int walk_submit(pa_encoder* e, int64_t data_bytes, const int64_t* entries, int32_t n_entries, int32_t cap_per_entry) {
    if (!e || !entries || n_entries < 1 || cap_per_entry < 1 || data_bytes < 0) return pa::set_error(PA_ERR_INVALID, "null or invalid argument");
    if (!e->variant || e->variant->resident_bytes <= 0 || data_bytes > e->variant->resident_bytes)
        return pa::set_error(PA_ERR_INVALID, "no inflated span of that size resident on the device");
    for (int32_t k = 0; k < n_entries; ++k)
        if (entries[k] < 0 || entries[k] > data_bytes || (k > 0 && entries[k] <= entries[k - 1]))
            return pa::set_error(PA_ERR_INVALID, "record entries must ascend inside the span");
    ENC_HIP(hipSetDevice(e->device));
    pa_variant_batch& b = *e->variant;
    b.walk.valid = b.pk.valid = false;
    hipStream_t st = e->stream;
    const size_t n = (size_t)n_entries, slots = n * (size_t)cap_per_entry;
    const size_t o_counts = n * 8, o_base = o_counts + n * 4, o_flags = o_base + (n + 1) * 4, o_slots = (o_flags + 8 + 63) & ~(size_t)63,
                 o_out = o_slots + slots * 40, total = o_out + slots * 40;
    ENC_ALLOC(b.d_walk, total);
    const size_t h_tail = (n * 8 + 63) & ~(size_t)63;
    if (!b.h_walk.ensure(h_tail + 64)) return pa::set_error(PA_ERR_HIP, "hipHostMalloc failed in the record walk");
    char* dw = b.d_walk.as<char>();
    char* hw = b.h_walk.as<char>();
    std::memcpy(hw, entries, n * 8);
    int32_t* tail = reinterpret_cast<int32_t*>(hw + h_tail);           // [0] the number of records, [1..2] the flags
    tail[0] = tail[1] = tail[2] = 0;
    // entries in and totals out through the page-locked block itself where it is mapped (see pa_encoder_inflate_bgzf)
    void* mapped = nullptr;
    if (hipHostGetDevicePointer(&mapped, hw, 0) != hipSuccess || !mapped) mapped = nullptr;
    char* mw = static_cast<char*>(mapped);
    b.walk.t0 = std::chrono::steady_clock::now();
    if (!mapped) ENC_HIP(hipMemcpyAsync(dw, hw, n * 8, hipMemcpyHostToDevice, st));
    ENC_HIP(hipMemsetAsync(dw + o_flags, 0, 8, st));
    pa::launch_record_walk(st, b.d_arena.as<uint8_t>(), data_bytes, reinterpret_cast<const int64_t*>(mapped ? mw : dw), n_entries,
                           cap_per_entry, dw + o_slots, reinterpret_cast<int32_t*>(dw + o_counts), reinterpret_cast<int32_t*>(dw + o_base),
                           reinterpret_cast<int32_t*>(dw + o_flags), dw + o_out, (int64_t)slots,
                           mapped ? reinterpret_cast<int32_t*>(mw + h_tail) : nullptr, e->split_walk ? 1 : 0);
    ENC_HIP(hipGetLastError());
    if (!mapped) {
        ENC_HIP(hipMemcpyAsync(tail, dw + o_base + n * 4, 4, hipMemcpyDeviceToHost, st));
        ENC_HIP(hipMemcpyAsync(tail + 1, dw + o_flags, 8, hipMemcpyDeviceToHost, st));
    }
    b.walk.mapped = mapped != nullptr;
    b.walk.slots = slots;
    b.walk.o_count = o_base + n * 4;
    b.walk.o_flags = o_flags;
    b.walk.o_out = o_out;
    b.walk.h_tail = h_tail;
    b.walk.valid = true;
    return PA_OK;
}

int pa_encoder_submit_walk(pa_encoder* e, int64_t data_bytes, const int64_t* entries, int32_t n_entries, int32_t cap_per_entry) {
    return walk_submit(e, data_bytes, entries, n_entries, cap_per_entry);
}

// the wait, the walk's tail words and, where they are clean, the headers themselves
int pa_encoder_walk_headers(pa_encoder* e, void* headers, int64_t headers_cap, int64_t* n_headers, int32_t* flags) {
    if (!e || !headers || headers_cap < 0 || !n_headers || !flags) return pa::set_error(PA_ERR_INVALID, "null or invalid argument");
    *n_headers = 0;
    flags[0] = flags[1] = 0;
    if (!e->variant || !e->variant->walk.valid) return pa::set_error(PA_ERR_INVALID, "no record walk of the resident span on this handle");
    ENC_HIP(hipSetDevice(e->device));
    pa_variant_batch& b = *e->variant;
    hipStream_t st = e->stream;
    const int32_t* tail = reinterpret_cast<const int32_t*>(b.h_walk.as<char>() + b.walk.h_tail);
    ENC_HIP(hipStreamSynchronize(st));
    flags[0] = tail[1];
    flags[1] = tail[2];
    const int64_t found = tail[0];
    if (flags[0] == 0 && found > headers_cap) flags[0] |= 4;            // the caller's table is too small
    if (flags[0] == 0 && found > 0) {                                   // (the headers themselves: one copy out of device memory --
        ENC_HIP(hipMemcpyAsync(headers, b.d_walk.as<char>() + b.walk.o_out, (size_t)found * 40, hipMemcpyDeviceToHost, st));      // 40-byte stores of single
        ENC_HIP(hipStreamSynchronize(st));                                                              // lanes across PCIe are slower)
    }
    *n_headers = flags[0] == 0 ? found : 0;
    return PA_OK;
}

int pa_encoder_walk_records(pa_encoder* e, int64_t data_bytes, const int64_t* entries, int32_t n_entries, int32_t cap_per_entry,
                            void* headers, int64_t headers_cap, int64_t* n_headers, int32_t* flags) {
    if (!e || !entries || n_entries < 1 || cap_per_entry < 1 || !headers || headers_cap < 0 || !n_headers || !flags || data_bytes < 0)
        return pa::set_error(PA_ERR_INVALID, "null or invalid argument");
    *n_headers = 0;
    flags[0] = flags[1] = 0;
    int rc = walk_submit(e, data_bytes, entries, n_entries, cap_per_entry);
    if (rc == PA_OK) rc = pa_encoder_walk_headers(e, headers, headers_cap, n_headers, flags);
    if (rc != PA_OK) return rc;
    pa_variant_batch& b = *e->variant;
    b.ms[11] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b.walk.t0).count();
    return PA_OK;
}

// The read and pair tables of a run of regions built where the headers lie (pack_scan_kernel, pack_fill_kernel): one
// submission -- behind the walk's, when pa_encoder_submit_walk has just queued it -- and one wait; the summary comes back
// through the page-locked block (mapped where possible, else one small copy)
int pa_encoder_pack_records(pa_encoder* e, const void* headers, int64_t n_headers, int32_t data_is_final, int32_t ref_id,
                            int32_t n_regions, const int64_t* start, const int64_t* stop, int32_t include_supplementary,
                            int32_t min_mapq, int32_t reads_cap, int32_t pairs_cap, int32_t* region_pairs, pa_device_pack* out) {
    if (!e || !out || !region_pairs || n_regions < 0 || (n_regions > 0 && (!start || !stop)) || n_headers < 0 || reads_cap < 0 ||
        pairs_cap < 0 || ref_id < 0)
        return pa::set_error(PA_ERR_INVALID, "null or invalid argument");
    *out = pa_device_pack{};
    for (int r = 0; r <= n_regions; ++r) region_pairs[r] = 0;
    for (int r = 0; r < n_regions; ++r)
        if (stop[r] < start[r] || (r > 0 && (start[r] < start[r - 1] || stop[r] < stop[r - 1])))
            return pa::set_error(PA_ERR_INVALID, "pack_records: regions must be ascending in start and stop");
    ENC_HIP(hipSetDevice(e->device));
    if (!e->variant) e->variant = new pa_variant_batch();
    pa_variant_batch& b = *e->variant;
    b.pk.valid = false;
    if (!headers && !b.walk.valid) return pa::set_error(PA_ERR_INVALID, "no headers given and no record walk of the resident span on this handle");
    if (n_regions == 0) return PA_OK;
    hipStream_t st = e->stream;
    const size_t nr = (size_t)n_regions, head_bytes = (pack_head_bytes(n_regions) + 15) & ~(size_t)15;
    // device state: head | start, stop | bases, operations, closed bytes [n] x 8 | pairs, closed reads [n] x 4
    const size_t o_bounds = head_bytes, o_rb = o_bounds + nr * 16, o_ro = o_rb + nr * 8, o_cb = o_ro + nr * 8, o_rp = o_cb + nr * 8,
                 o_cr = o_rp + nr * 4, state_bytes = o_cr + nr * 4;
    ENC_ALLOC(b.d_pk_state, state_bytes + 64);
    ENC_ALLOC(b.d_pk_reads, (size_t)reads_cap * sizeof(PackedRead) + 64);
    ENC_ALLOC(b.d_pk_soff, (size_t)reads_cap * 8 + 64);
    ENC_ALLOC(b.d_pk_range, (size_t)reads_cap * 8 + 64);
    ENC_ALLOC(b.d_pk_pairs, (size_t)pairs_cap * sizeof(PairRec) + 64);
    ENC_ALLOC(b.d_pk_pair_read, (size_t)pairs_cap * 4 + 64);
    if (headers) ENC_ALLOC(b.d_pk_hdr, (size_t)n_headers * sizeof(PackHdr) + 64);
    // page-locked: start, stop | head
    if (!b.h_pk.ensure(nr * 16 + head_bytes)) return pa::set_error(PA_ERR_HIP, "hipHostMalloc failed in the device pack");
    char* hp = b.h_pk.as<char>();
    std::memcpy(hp, start, nr * 8);
    std::memcpy(hp + nr * 8, stop, nr * 8);
    pa_device_pack* hsum = reinterpret_cast<pa_device_pack*>(hp + nr * 16);
    *hsum = pa_device_pack{};
    hsum->status = -1;                              // (a kernel that never ran leaves no usable summary)
    void* mapped = nullptr;
    if (hipHostGetDevicePointer(&mapped, hp, 0) != hipSuccess || !mapped) mapped = nullptr;
    char* ds = b.d_pk_state.as<char>();
    if (headers && n_headers > 0)
        ENC_HIP(hipMemcpyAsync(b.d_pk_hdr.p, headers, (size_t)n_headers * sizeof(PackHdr), hipMemcpyHostToDevice, st));
    if (!mapped) ENC_HIP(hipMemcpyAsync(ds + o_bounds, hp, nr * 16, hipMemcpyHostToDevice, st));
    PackArgs a{};
    if (headers) {
        a.hdr = b.d_pk_hdr.as<PackHdr>();
        a.n_hdr = n_headers;
    } else {
        const char* dw = b.d_walk.as<char>();
        a.hdr = reinterpret_cast<const PackHdr*>(dw + b.walk.o_out);
        a.n_hdr_dev = reinterpret_cast<const int32_t*>(dw + b.walk.o_count);
        a.walk_flags_dev = reinterpret_cast<const int32_t*>(dw + b.walk.o_flags);
        a.hdr_cap = (int64_t)b.walk.slots;
    }
    a.bounds = reinterpret_cast<int64_t*>(ds + o_bounds);
    a.bounds_src = mapped ? static_cast<const int64_t*>(mapped) : a.bounds;
    a.n_regions = n_regions;
    a.tid = ref_id;
    a.is_final = data_is_final != 0;
    a.include_supplementary = include_supplementary;
    a.min_mapq = min_mapq;
    a.split = e->split_walk ? 1 : 0;
    a.reads_cap = reads_cap;
    a.pairs_cap = pairs_cap;
    a.span_bytes = b.resident_bytes;
    a.reads = b.d_pk_reads.as<PackedRead>();
    a.seq_off = b.d_pk_soff.as<int64_t>();
    a.range = b.d_pk_range.as<int2>();
    a.pairs = b.d_pk_pairs.as<PairRec>();
    a.pair_read = b.d_pk_pair_read.as<int32_t>();
    a.r_bases = reinterpret_cast<unsigned long long*>(ds + o_rb);
    a.r_ops = reinterpret_cast<unsigned long long*>(ds + o_ro);
    a.closed_bytes = reinterpret_cast<int64_t*>(ds + o_cb);
    a.r_pairs = reinterpret_cast<int32_t*>(ds + o_rp);
    a.closed_reads = reinterpret_cast<int32_t*>(ds + o_cr);
    a.head = reinterpret_cast<int32_t*>(ds);
    a.head_mapped = mapped ? reinterpret_cast<int32_t*>(static_cast<char*>(mapped) + nr * 16) : nullptr;
    a.head_words = (int32_t)(pack_head_bytes(n_regions) / 4);
    hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(PACK_BLOCK), 0, st, a);
    ENC_HIP(hipGetLastError());
    hipLaunchKernelGGL(pack_fill_kernel, dim3((unsigned)n_regions), dim3(PACK_BLOCK), 0, st, a);
    ENC_HIP(hipGetLastError());
    if (!mapped) ENC_HIP(hipMemcpyAsync(hp + nr * 16, ds, pack_head_bytes(n_regions), hipMemcpyDeviceToHost, st));
    ENC_HIP(hipStreamSynchronize(st));
    if (hsum->status < 0) return pa::set_error(PA_ERR_HIP, "the device pack left no summary");
    *out = *hsum;
    const int32_t* h_pairs = reinterpret_cast<const int32_t*>(hp + nr * 16 + 64);
    const int32_t* h_ops = reinterpret_cast<const int32_t*>(hp + nr * 16 + pack_head_ops(n_regions));
    const int64_t* h_bases = reinterpret_cast<const int64_t*>(hp + nr * 16 + pack_head_bases(n_regions));
    if (out->status == 0) {
        std::copy(h_pairs, h_pairs + nr + 1, region_pairs);
        b.pk.sum = *out;
        b.pk.region_pairs.assign(h_pairs, h_pairs + nr + 1);
        b.pk.op_base.assign(h_ops, h_ops + nr + 1);
        b.pk.seq_base.assign(h_bases, h_bases + nr + 1);
        b.pk.valid = true;
        b.pk.on_device += 1;
    } else {
        b.pk.handed_back += 1;
    }
    if (!headers) b.ms[11] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b.walk.t0).count();
    return PA_OK;
}

int pa_encoder_stage_packed_device(pa_encoder* e, int32_t n_regions, const pa_packed_region* regions, const pa_summary_params* params) {
    if (!e || !e->variant || !e->variant->pk.valid) return pa::set_error(PA_ERR_INVALID, "no tables packed on the device for the resident span");
    pa_variant_batch& b = *e->variant;
    if (n_regions != b.pk.sum.n_done) return pa::set_error(PA_ERR_INVALID, "the device pack closed another number of regions");
    return stage_packed_device(e, n_regions, regions, params);
}

int pa_encoder_packed_tables(pa_encoder* e, pa_packed_read* reads, int32_t* pair_read, int64_t* seq_off) {
    if (!e || !e->variant || !e->variant->pk.valid) return pa::set_error(PA_ERR_INVALID, "no tables packed on the device");
    ENC_HIP(hipSetDevice(e->device));
    pa_variant_batch& b = *e->variant;
    const size_t n_reads = (size_t)b.pk.sum.n_reads, n_pairs = (size_t)b.pk.sum.n_pairs;
    if (reads && n_reads) ENC_HIP(hipMemcpyAsync(reads, b.d_pk_reads.p, n_reads * sizeof(PackedRead), hipMemcpyDeviceToHost, e->stream));
    if (seq_off && n_reads) ENC_HIP(hipMemcpyAsync(seq_off, b.d_pk_soff.p, n_reads * 8, hipMemcpyDeviceToHost, e->stream));
    if (pair_read && n_pairs) ENC_HIP(hipMemcpyAsync(pair_read, b.d_pk_pair_read.p, n_pairs * 4, hipMemcpyDeviceToHost, e->stream));
    ENC_HIP(hipStreamSynchronize(e->stream));
    return PA_OK;
}

int pa_encoder_pack_calls(pa_encoder* e, int64_t* on_device, int64_t* handed_back) {
    if (!e) return pa::set_error(PA_ERR_INVALID, "null encoder");
    if (on_device) *on_device = e->variant ? e->variant->pk.on_device : 0;
    if (handed_back) *handed_back = e->variant ? e->variant->pk.handed_back : 0;
    return PA_OK;
}

int pa_encoder_stage_packed(pa_encoder* e, int32_t n_regions, const pa_packed_region* regions, const pa_summary_params* params,
                            const uint8_t* arena, int64_t arena_bytes, const pa_packed_read* reads, int32_t n_reads,
                            const int32_t* pair_read, const int32_t* region_pairs) {
    return stage_packed(e, n_regions, regions, params, arena, arena_bytes, reads, n_reads, pair_read, region_pairs);
}

int pa_encoder_set_split_slices(pa_encoder* e, int32_t on) {
    if (!e) return pa::set_error(PA_ERR_INVALID, "null encoder");
    e->split_walk = on != 0;
    return PA_OK;
}

int pa_encoder_set_seq_offsets(pa_encoder* e, const int64_t* seq_off, int32_t n_reads) {
    if (!e || n_reads < 0 || (n_reads > 0 && !seq_off)) return pa::set_error(PA_ERR_INVALID, "null argument");
    e->seq_off.assign(seq_off, seq_off + n_reads);
    return PA_OK;
}

int pa_encoder_set_host_threads(pa_encoder* e, int32_t n) {
    if (!e || n < 0) return pa::set_error(PA_ERR_INVALID, "null encoder or negative thread count");
    if (!e->variant) e->variant = new pa_variant_batch();
    e->variant->host_threads = n;
    e->variant->pool.reset();
    return PA_OK;
}

int pa_encoder_set_device_candidates(pa_encoder* e, int32_t on) {
    if (!e) return pa::set_error(PA_ERR_INVALID, "null encoder");
    if (!e->variant) e->variant = new pa_variant_batch();
    e->variant->dev_cands = on != 0;
    return PA_OK;
}

int pa_encoder_set_targets(pa_encoder* e, int64_t n, const int64_t* start, const int64_t* end) {
    if (!e || n < 0 || (n > 0 && (!start || !end))) return pa::set_error(PA_ERR_INVALID, "null argument");
    if (n > ((int64_t)1 << 28)) return pa::set_error(PA_ERR_INVALID, "targets: more than 2^28 intervals");
    for (int64_t i = 0; i < n; ++i)                // (checked in full before anything of the handle changes)
        if (start[i] < 0 || start[i] >= end[i] || (i > 0 && start[i] <= end[i - 1]))
            return pa::set_error(PA_ERR_INVALID, "targets: interval " + std::to_string(i) +
                                                     " is empty, negative, or not behind the end of the one before it");
    if (n == 0) {
        e->n_targets = 0;
        return PA_OK;
    }
    ENC_HIP(hipSetDevice(e->device));
    e->n_targets = 0;                              // (no table while the buffer may move)
    ENC_ALLOC(e->d_target_table, (size_t)n * 16);
    int64_t* tab = e->d_target_table.as<int64_t>();
    ENC_HIP(hipMemcpyAsync(tab, start, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    ENC_HIP(hipMemcpyAsync(tab + n, end, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    ENC_HIP(hipStreamSynchronize(e->stream));
    e->n_targets = n;
    return PA_OK;
}

int pa_encoder_set_depth_bins(pa_encoder* e, int32_t n, const int32_t* lower) {
    if (!e || n < 0 || (n > 0 && !lower)) return pa::set_error(PA_ERR_INVALID, "null argument");
    if (n > TRACK_CLASSES) return pa::set_error(PA_ERR_INVALID, "depth bins: entry 8 is one more than the 8 bins a table may have");
    for (int32_t k = 0; k < n; ++k)                // (checked in full before anything of the handle changes)
        if (k == 0 ? lower[0] != 0 : lower[k] <= lower[k - 1])
            return pa::set_error(PA_ERR_INVALID, "depth bins: entry " + std::to_string(k) +
                                                     (k == 0 ? " must be 0" : " is not above the one before it"));
    e->depth_bins.set(n, lower, "PEPPER_AMD_DEPTH_RUN_CAP");     // (the capacity is for debugging: tests/test_gpu_coverage.py makes a run overflow with it)
    return PA_OK;
}

int pa_encoder_depth_runs(pa_encoder* e, int64_t capacity, int32_t* region, int64_t* start, int64_t* end, int32_t* bin, int64_t* n_runs) {
    if (!e || capacity < 0) return pa::set_error(PA_ERR_INVALID, "null argument");
    if (!e->variant || !e->variant->depth.on) return pa::set_error(PA_ERR_INVALID, "depth runs: the handle's last run had no depth bins set");
    return fetch_track<DepthRun>(e, e->variant->depth, "depth runs", "runs", region || start || end || bin, capacity, region, start, end, n_runs,
                                 [&](size_t k, const DepthRun& r) { if (bin) bin[k] = reported_class(r.bin); });
}

int pa_encoder_depth_totals(pa_encoder* e, int32_t n_regions, int64_t* bases, int64_t* depth_sum) {
    if (!e || n_regions < 0) return pa::set_error(PA_ERR_INVALID, "null argument");
    if (!e->variant || !e->variant->depth.on) return pa::set_error(PA_ERR_INVALID, "depth totals: the handle's last run had no depth bins set");
    pa_variant_batch& b = *e->variant;
    if (n_regions > (int32_t)b.regs.size()) return pa::set_error(PA_ERR_INVALID, "depth totals: more regions than the last run had");
    const unsigned long long* tot = b.h_dtot.as<unsigned long long>();
    for (int32_t r = 0; r < n_regions; ++r) {
        if (bases)
            for (int k = 0; k < TRACK_CLASSES; ++k) bases[(size_t)r * TRACK_CLASSES + k] = (int64_t)tot[(size_t)r * DEPTH_TOTALS + k];
        if (depth_sum) depth_sum[r] = (int64_t)tot[(size_t)r * DEPTH_TOTALS + TRACK_CLASSES];
    }
    return PA_OK;
}

int pa_encoder_depth_calls(pa_encoder* e, int64_t* runs_with_bins, int64_t* overflows) {
    return track_calls(e, &pa_variant_batch::depth, runs_with_bins, overflows);
}

int pa_encoder_set_ref_confidence(pa_encoder* e, const uint8_t* table, int32_t table_side, int32_t n_bands, const int32_t* lower) {
    if (!e || n_bands < 0 || (n_bands > 0 && (!lower || !table))) return pa::set_error(PA_ERR_INVALID, "null argument");
    if (n_bands == 0) {
        e->ref_bands.n = 0;
        e->ref_bands.cap = 0;
        return PA_OK;
    }
    // (checked in full before anything of the handle changes)
    if (table_side != REFCONF_SIDE)
        return pa::set_error(PA_ERR_INVALID, "reference confidence: a table of side " + std::to_string(table_side) + ", not " +
                                                 std::to_string(REFCONF_SIDE));
    if (n_bands > TRACK_CLASSES)
        return pa::set_error(PA_ERR_INVALID, "reference confidence: band 8 is one more than the 8 bands a table may have");
    for (int32_t k = 0; k < n_bands; ++k)
        if (k == 0 ? lower[0] != 0 : (lower[k] <= lower[k - 1] || lower[k] > 255))
            return pa::set_error(PA_ERR_INVALID, "reference confidence: band " + std::to_string(k) +
                                                     (k == 0 ? " must start at 0" : lower[k] > 255 ? " is above 255, the largest GQ a table holds"
                                                                                                   : " is not above the one before it"));
    if (table[0] != 0) return pa::set_error(PA_ERR_INVALID, "reference confidence: table entry (0, 0) must be 0: no read, no confidence");
    // more reference reads never lower the confidence, more other reads never raise it
    for (int r = 0; r < REFCONF_SIDE; ++r)
        for (int a = 0; a < REFCONF_SIDE; ++a) {
            const int v = table[r * REFCONF_SIDE + a];
            if ((r > 0 && v < table[(r - 1) * REFCONF_SIDE + a]) || (a > 0 && v > table[r * REFCONF_SIDE + a - 1]))
                return pa::set_error(PA_ERR_INVALID, "reference confidence: table entry (" + std::to_string(r) + ", " + std::to_string(a) +
                                                         ") is not monotone: GQ rises with n_ref and falls with n_alt");
        }
    ENC_HIP(hipSetDevice(e->device));
    ENC_HIP(hipStreamSynchronize(e->stream));      // (no run of the handle reads the table while it changes)
    ENC_ALLOC(e->d_gq_table, (size_t)REFCONF_SIDE * REFCONF_SIDE);
    ENC_HIP(hipMemcpyAsync(e->d_gq_table.p, table, (size_t)REFCONF_SIDE * REFCONF_SIDE, hipMemcpyHostToDevice, e->stream));
    ENC_HIP(hipStreamSynchronize(e->stream));
    e->ref_bands.set(n_bands, lower, "PEPPER_AMD_REF_BLOCK_CAP");     // (the capacity is for debugging: tests/test_gpu_refconf.py makes a run overflow with it)
    return PA_OK;
}

int pa_encoder_ref_blocks(pa_encoder* e, int64_t capacity, int32_t* region, int64_t* start, int64_t* end, int32_t* band, int32_t* min_dp,
                          int32_t* min_gq, int64_t* n_blocks) {
    if (!e || capacity < 0) return pa::set_error(PA_ERR_INVALID, "null argument");
    if (!e->variant || !e->variant->blocks.on)
        return pa::set_error(PA_ERR_INVALID, "reference blocks: the handle's last run had no reference-confidence table set");
    return fetch_track<RefBlock>(e, e->variant->blocks, "reference blocks", "blocks", region || start || end || band || min_dp || min_gq,
                                 capacity, region, start, end, n_blocks, [&](size_t k, const RefBlock& r) {
                                     if (band) band[k] = reported_class(r.band);
                                     if (min_dp) min_dp[k] = r.min_dp;
                                     if (min_gq) min_gq[k] = r.min_gq;
                                 });
}

int pa_encoder_ref_calls(pa_encoder* e, int64_t* runs, int64_t* overflows) {
    return track_calls(e, &pa_variant_batch::blocks, runs, overflows);
}

int pa_encoder_candidate_calls(pa_encoder* e, int64_t* on_device, int64_t* on_host) {
    if (!e) return pa::set_error(PA_ERR_INVALID, "null encoder");
    if (on_device) *on_device = e->variant ? e->variant->dev_calls : 0;
    if (on_host) *on_host = e->variant ? e->variant->host_calls : 0;
    return PA_OK;
}

int pa_encoder_region_reads(pa_encoder* e, int32_t* n_reads, int32_t n) {
    if (!e || !n_reads || n < 0) return pa::set_error(PA_ERR_INVALID, "null argument");
    for (int i = 0; i < n; ++i) n_reads[i] = (e->variant && i < (int)e->variant->live.size()) ? e->variant->live[(size_t)i] : 0;
    return PA_OK;
}

int pa_encoder_set_sampling(pa_encoder* e, uint32_t seed, int32_t max_reads, double rate) {
    if (!e) return pa::set_error(PA_ERR_INVALID, "null encoder");
    if (max_reads < 0 || max_reads > RS_CAP || !(rate >= 0.0))
        return pa::set_error(PA_ERR_INVALID, "sampling: 0 <= max_reads <= 5000 (0 switches it off) and rate >= 0");
    e->sampler.on = max_reads > 0;
    e->sampler.seed = seed;
    e->sampler.cap = max_reads;
    e->sampler.rate = rate;
    return PA_OK;
}

int pa_encoder_sampled_regions(pa_encoder* e, int64_t* regions, int64_t* reads_dropped) {
    if (!e) return pa::set_error(PA_ERR_INVALID, "null encoder");
    if (regions) *regions = e->sampler.regions;
    if (reads_dropped) *reads_dropped = e->sampler.dropped;
    return PA_OK;
}

int pa_encoder_pair_live(pa_encoder* e, uint8_t* keep, int64_t n) {
    if (!e || n < 0 || (n > 0 && !keep)) return pa::set_error(PA_ERR_INVALID, "null argument");
    if (!e->variant || n > e->variant->last_pairs) return pa::set_error(PA_ERR_INVALID, "no packed batch with that many pairs");
    if (n == 0) return PA_OK;
    ENC_HIP(hipSetDevice(e->device));
    std::vector<ReadRec> reads((size_t)n);
    ENC_HIP(hipMemcpyAsync(reads.data(), e->variant->d_reads.p, (size_t)n * sizeof(ReadRec), hipMemcpyDeviceToHost, e->stream));
    ENC_HIP(hipStreamSynchronize(e->stream));
    for (int64_t p = 0; p < n; ++p) keep[p] = reads[(size_t)p].slen > 0 ? 1 : 0;
    return PA_OK;
}

int pa_encoder_generate_summary_batch(pa_encoder* e, int32_t n_regions, const pa_pileup* pileups, const pa_summary_params* params,
                                      int64_t* n_candidates) {
    const int rc = stage_batch(e, n_regions, pileups, params);
    return rc != PA_OK ? rc : run_staged(e, n_candidates);
}

int pa_encoder_generate_summary(pa_encoder* e, const pa_pileup* p, const pa_summary_params* q, int64_t* n_candidates) {
    if (!e || !p || !q || !n_candidates) return pa::set_error(PA_ERR_INVALID, "null argument");
    return pa_encoder_generate_summary_batch(e, 1, p, q, n_candidates);
}

int pa_encoder_get_results(pa_encoder* e, int64_t* positions, int32_t* depths, int32_t* candidate_frequency,
                           int32_t* images_i32, int8_t* images_i8, char* candidates, int64_t candidates_cap,
                           int64_t* candidates_needed) {
    if (!e) return pa::set_error(PA_ERR_INVALID, "null encoder");
    ENC_HIP(hipSetDevice(e->device));
    if (!e->variant) {
        if (candidates_needed) *candidates_needed = 0;
        return PA_OK;
    }
    pa_variant_batch& b = *e->variant;
    const size_t n = (size_t)b.n;
    if (b.dev_results) {              // enumerated on the device: the lists are fetched when somebody asks for them
        b.positions.assign(n, 0);
        b.depths.assign(n, 0);
        b.freqs.assign(n, 0);
        b.names.assign((size_t)b.name_bytes, '\0');
        if (n > 0) {
            ENC_HIP(hipMemcpyAsync(b.positions.data(), b.d_pos.p, n * 8, hipMemcpyDeviceToHost, e->stream));
            ENC_HIP(hipMemcpyAsync(b.depths.data(), b.d_depths.p, n * 4, hipMemcpyDeviceToHost, e->stream));
            ENC_HIP(hipMemcpyAsync(b.freqs.data(), b.d_freqs.p, n * 4, hipMemcpyDeviceToHost, e->stream));
            ENC_HIP(hipMemcpyAsync(&b.names[0], b.d_names.p, (size_t)b.name_bytes, hipMemcpyDeviceToHost, e->stream));
            ENC_HIP(hipStreamSynchronize(e->stream));
        }
        b.dev_results = false;
    }
    if (positions) std::copy(b.positions.begin(), b.positions.end(), positions);
    if (depths) std::copy(b.depths.begin(), b.depths.end(), depths);
    if (candidate_frequency) std::copy(b.freqs.begin(), b.freqs.end(), candidate_frequency);
    if (candidates_needed) *candidates_needed = (int64_t)b.names.size();
    if (candidates && candidates_cap >= (int64_t)b.names.size()) std::memcpy(candidates, b.names.data(), b.names.size());
    if (n > 0 && images_i32)
        ENC_HIP(hipMemcpyAsync(images_i32, b.d_img32.p, n * b.W * b.F * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    if (n > 0 && images_i8)
        ENC_HIP(hipMemcpyAsync(images_i8, b.d_img8.p, n * b.W * b.F, hipMemcpyDeviceToHost, e->stream));
    ENC_HIP(hipStreamSynchronize(e->stream));
    return PA_OK;
}

const int8_t* pa_encoder_device_images(pa_encoder* e) {
    return (e && e->variant && e->variant->n > 0) ? e->variant->d_img8.as<int8_t>() : nullptr;
}

int pa_encoder_last_timing(pa_encoder* e, double* ms, int32_t n) {
    if (!e || !ms || n < 0) return pa::set_error(PA_ERR_INVALID, "null argument");
    for (int i = 0; i < n; ++i) ms[i] = (e->variant && i < 15) ? e->variant->ms[i] : 0.0;
    return PA_OK;
}

int pa_encoder_batch_stats(pa_encoder* e, int64_t* out, int32_t n) {
    if (!e || !out || n < 0) return pa::set_error(PA_ERR_INVALID, "null argument");
    const int64_t v[6] = {e->variant ? e->variant->total_bases : 0, e->variant ? e->variant->total_rows : 0,
                          e->variant ? e->variant->total_reads : 0, e->variant ? e->variant->total_ops : 0,
                          e->variant ? (int64_t)e->variant->n_tiles : 0, e->variant ? (int64_t)e->variant->regs.size() : 0};
    for (int i = 0; i < n; ++i) out[i] = i < 6 ? v[i] : 0;
    return PA_OK;
}

}  // extern "C"
