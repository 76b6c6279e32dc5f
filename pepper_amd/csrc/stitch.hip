// Polish stitch on the device (include/pepper_amd_encoder.h, pa_stitcher_*).
//
// replaces, for a run that opts in: the merge of pepper/modules/python/Stitch.py small_chunk_stitch (:36-94) -- per piece a
// dictionary keyed (position, insert index), written in loop order, the last write of a key wins, keys come out sorted, gaps
// are dropped -- which pa_h5_stitch_polish_regions runs on CPU cores from the prediction files.
//
// The merge needs no sort.  A piece's keys are dense: positions span [first, last] and a position holds max(index) + 1 keys, so
//   width[piece, position] = max(index) + 1              (atomicMax)
//   base                   = exclusive scan of the widths  (the slot of key (position, 0))
//   slot[base + index]     = max over its writers of ((rank + 1) << 16 | phred << 8 | label)    (64-bit atomicMax)
// where rank numbers the kept rows of the contig in the reference's loop order.  Ranks are distinct, so the rank alone decides
// the maximum and the phred and the label of the winner ride along.  An integer maximum does not depend on the
// order the rows arrive in, so the winner is the dictionary's last write whatever the schedule.  A second scan over "the winner is
// a base" gives every letter its place.  Both scans are reduce-then-scan over separate launches (block sums, scan of the sums,
// add back): no workgroup ever waits for another one.
//
// add() is the streaming half: a count kernel and a compaction kernel per call keep the rows the dictionary would take (stored
// order), 8 bytes each, in fixed-size slabs that are never moved.
//
// Qualities (pa_stitcher_add_qual, pa_stitcher_take_qualities): a row added with its phred carries it above the position, the
// scatter word carries it between the rank and the label, and the emit that places the letters places, from the same winner,
// chr(33 + min(phred, 93)) into a second buffer -- no further scan, no further wait.
//
// Edits (pa_stitcher_edits, pa_stitcher_take_edits; opt-in, not in the reference): what the consensus changed against the draft,
// read off the tables the last finish left.  One lane per SLOT (not per position: a position with thousands of insert slots
// spreads over as many lanes); a lane finds its position by bisecting the slot bases, so it needs no table of its own.  A slot
// gives 0 or 1 record, and the slot (p, 0) behind a run of uncovered positions carries the run's two GAP records in front of
// its own: every run is closed by exactly one such slot.  Count (block sums), scan of the sums, write: the write pass scans
// its block again instead of reading a per-slot prefix, so the only table this adds is the records themselves.
//
// Fill (pa_stitcher_fill; opt-in, not in the reference): the consensus of a finish with ONE piece, completed with the draft's own
// letters where a position has no slot -- in front of the piece, behind it, and in the runs inside it.  One more exclusive scan,
// over "the position has no slot" (the same reduce-then-scan), tells every position how many draft letters lie in front of it
// inside the piece; the scanned word also counts, in its upper half, the positions that begin a run, so the one total that comes
// back sizes the buffer and counts the runs.  Then one lane per POSITION writes what the position gives: its slots' letters at
// lead + place + holes, or draft[p] (and '!') at lead + letters in front + holes.  The two ends are copies of the draft.
//
// Gate (pa_stitcher_gate, pa_stitcher_take_withheld; opt-in, not in the reference): only the edits against the draft whose winner
// has a phred of at least min_phred are applied; the others are withheld -- the slot emits the draft's letter (SUB, DEL) or nothing
// (INS) with phred 0 -- and listed.  Runs behind a finish, in front of fill and edits.  One lane per slot, twice: the first pass
// decides from the winner word and the draft, rewrites letters[] and counts; the letters are scanned again; the second pass
// decides once more (the words still hold the model's labels), places the records (count, scan, write) and rewrites the words, so
// emit, fill and edits read consistent tables without knowing about the gate.  A lane touches only its own slot.
//
// Variants (pa_stitcher_variants, pa_stitcher_take_variants; opt-in, not in the reference): the edit records of the FILLED consensus
// grouped into hunks, trimmed and left-aligned against the draft (the rule: the header, at the call).  Runs behind fill on what is
// resident: the draft, the filled consensus, the sorted records.  Hunk heads are decided inside a scan's load from a record and the
// one in front of it; a lane per record writes the hunks' ranges, a lane per hunk trims, a WAVE per hunk left-aligns -- one
// comparison per lane and a ballot for the first mismatch, 64 places per step, where a lane per hunk would walk a satellite
// repeat alone -- and a scan of "the hunk gives a record" compacts in hunk order.  A hunk reads its neighbour's trimmed and untrimmed
// ends, never its result; integer minima and sums only.
#include "../../include/pepper_amd.h"
#include "../../include/pepper_amd_encoder.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "kernels.h"
#include "scan.h"

namespace {

// ST_THREADS, ST_ITEMS, ST_B (scan elements per workgroup: pa_stitcher_limits [2]): scan.h
constexpr int64_t ST_SLAB_ROWS = 1 << 20;               // packed rows per slab: 8 MiB (pa_stitcher_limits [3])
constexpr int64_t ST_MAX_POSITION = 0xFFFFFFFFll;
constexpr int64_t ST_MAX_INDEX = 0xFFFFll;
constexpr uint64_t ST_MAX_ROWS = (1ull << 48) - 1;      // rank + 1 has 48 bits of the scatter word
constexpr uint32_t ST_MAX_QUALITY = 93;                 // Sanger: '!' + 93 = '~'

// packed row: phred << 56 | position << 24 | index << 8 | label
PA_DEV uint64_t pack_row(int64_t p, int64_t x, uint8_t label, uint8_t phred) {
    return ((uint64_t)phred << 56) | ((uint64_t)p << 24) | ((uint64_t)x << 8) | label;
}
PA_DEV uint32_t row_position(uint64_t v) { return (uint32_t)(v >> 24); }
PA_DEV uint32_t row_index(uint64_t v) { return (uint32_t)(v >> 8) & 0xFFFFu; }
PA_DEV uint32_t row_label(uint64_t v) { return (uint32_t)v & 0xFFu; }
PA_DEV uint32_t row_phred(uint64_t v) { return (uint32_t)(v >> 56); }

// the rows small_chunk_stitch keeps: position >= 0, index >= 0, and past the overlap of a region that does not start at 0
// (drop_below = start + 2 * MIN_IMAGE_OVERLAP there, -1 elsewhere)
PA_DEV bool keeps(int64_t p, int64_t x, int64_t drop_below) { return p >= 0 && x >= 0 && p > drop_below; }

// ---------------------------------------------------------------- add: count, then compact ----
__global__ __launch_bounds__(ST_THREADS) void k_stitch_count(const int64_t* __restrict__ pos, const int64_t* __restrict__ idx,
                                                             const int64_t* __restrict__ drop_below, int chunk_len,
                                                             int32_t* __restrict__ kept, int32_t* __restrict__ refused) {
    __shared__ int s_kept, s_bad;
    const int c = blockIdx.x;
    if (threadIdx.x == 0) s_kept = s_bad = 0;
    __syncthreads();
    const int64_t thr = drop_below[c];
    const size_t at = (size_t)c * chunk_len;
    int mine = 0, bad = 0;
    for (int i = threadIdx.x; i < chunk_len; i += ST_THREADS) {
        const int64_t p = pos[at + i], x = idx[at + i];
        if (keeps(p, x, thr)) {
            ++mine;
            bad |= (p > ST_MAX_POSITION || x > ST_MAX_INDEX);
        }
    }
    for (int d = 32; d; d >>= 1) {
        mine += __shfl_xor(mine, d);
        bad |= __shfl_xor(bad, d);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_kept, mine);
        if (bad) atomicOr(&s_bad, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        kept[c] = s_kept;
        refused[c] = s_bad;
    }
}

__global__ __launch_bounds__(ST_THREADS) void k_stitch_compact(const int64_t* __restrict__ pos, const int64_t* __restrict__ idx,
                                                               const uint8_t* __restrict__ labels, const uint8_t* __restrict__ phred,
                                                               const int64_t* __restrict__ drop_below, int chunk_len,
                                                               const int32_t* __restrict__ kept,
                                                               uint64_t* const* __restrict__ dst_of) {
    __shared__ int s_wave[ST_THREADS / 64];
    const int c = blockIdx.x;
    const int room = kept[c];
    if (room == 0) return;                               // (uniform for the workgroup)
    uint64_t* dst = dst_of[c];
    const int64_t thr = drop_below[c];
    const size_t at = (size_t)c * chunk_len;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int t = 0; t < chunk_len; t += ST_THREADS) {
        const int i = t + threadIdx.x;
        int64_t p = -1, x = -1;
        if (i < chunk_len) {
            p = pos[at + i];
            x = idx[at + i];
        }
        const bool keep = i < chunk_len && keeps(p, x, thr);
        const unsigned long long mask = __ballot(keep);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int wave_base = 0, total = 0;
        for (int w = 0; w < ST_THREADS / 64; ++w) {
            if (w < wave) wave_base += s_wave[w];
            total += s_wave[w];
        }
        const int o = base + wave_base + before;
        if (keep && o < room) dst[o] = pack_row(p, x, labels[at + i], phred ? phred[at + i] : (uint8_t)0);      // (phred: uniform)
        base += total;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- finish ----
struct ChunkDesc {                                      // one chunk of the contig, in loop order
    const uint64_t* rows;
    uint32_t count, piece;
    uint64_t rank_base;                                 // rank of its first kept row
};

__global__ __launch_bounds__(ST_THREADS) void k_stitch_range(const ChunkDesc* __restrict__ desc, uint32_t* __restrict__ pmin,
                                                             uint32_t* __restrict__ pmax) {
    const ChunkDesc d = desc[blockIdx.x];
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (uint32_t r = threadIdx.x; r < d.count; r += ST_THREADS) {
        const uint32_t p = row_position(d.rows[r]);
        lo = min(lo, p);
        hi = max(hi, p);
    }
    for (int s = 32; s; s >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, s));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, s));
    }
    if ((threadIdx.x & 63) == 0 && lo <= hi) {          // one pair of atomics per wave that saw a row
        atomicMin(&pmin[d.piece], lo);
        atomicMax(&pmax[d.piece], hi);
    }
}

__global__ __launch_bounds__(ST_THREADS) void k_stitch_width(const ChunkDesc* __restrict__ desc, const uint32_t* __restrict__ pmin,
                                                             const uint64_t* __restrict__ pbase, uint32_t* __restrict__ width,
                                                             uint64_t n_positions, uint32_t* __restrict__ fault) {
    const ChunkDesc d = desc[blockIdx.x];
    const uint64_t base = pbase[d.piece];
    const uint32_t first = pmin[d.piece];
    for (uint32_t r = threadIdx.x; r < d.count; r += ST_THREADS) {
        const uint64_t v = d.rows[r];
        const uint64_t at = base + (row_position(v) - first);
        if (at < n_positions) atomicMax(&width[at], row_index(v) + 1u);
        else atomicOr(fault, 1u);
    }
}

__global__ __launch_bounds__(ST_THREADS) void k_stitch_scatter(const ChunkDesc* __restrict__ desc, const uint32_t* __restrict__ pmin,
                                                               const uint64_t* __restrict__ pbase, const uint32_t* __restrict__ slot_base,
                                                               unsigned long long* __restrict__ slots, uint64_t n_positions,
                                                               uint64_t n_slots, uint32_t* __restrict__ fault) {
    const ChunkDesc d = desc[blockIdx.x];
    const uint64_t base = pbase[d.piece];
    const uint32_t first = pmin[d.piece];
    for (uint32_t r = threadIdx.x; r < d.count; r += ST_THREADS) {
        const uint64_t v = d.rows[r];
        const uint64_t at = base + (row_position(v) - first);
        uint64_t slot = n_slots;
        if (at < n_positions) slot = (uint64_t)slot_base[at] + row_index(v);
        if (slot < n_slots)
            atomicMax(&slots[slot], (unsigned long long)(((d.rank_base + r + 1) << 16) | ((uint64_t)row_phred(v) << 8) | row_label(v)));
        else atomicOr(fault, 2u);
    }
}

// the winner of every slot: its letter (0: a gap, an empty slot or a label that is no base), the largest label above 4
__global__ __launch_bounds__(ST_THREADS) void k_stitch_check(const unsigned long long* __restrict__ slots, uint64_t n_slots,
                                                             uint8_t* __restrict__ letters, uint32_t* __restrict__ bad_label) {
    const uint64_t i = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= n_slots) return;
    const uint32_t label = (uint32_t)slots[i] & 0xFFu;
    uint8_t letter = 0;
    if (label >= 1 && label <= 4) letter = (uint8_t)((0x54474341u >> (8 * (label - 1))) & 0xFFu);      // "ACGT"
    else if (label > 4) atomicMax(bad_label, label);
    letters[i] = letter;
}

// QUAL: the winner's phred, clamped and offset, goes to the letter's place in `qual` as well
template <bool QUAL>
__global__ __launch_bounds__(ST_THREADS) void k_stitch_emit(const uint8_t* __restrict__ letters, const uint32_t* __restrict__ place,
                                                            const unsigned long long* __restrict__ slots, uint64_t n_slots,
                                                            uint64_t n_letters, uint8_t* __restrict__ out, uint8_t* __restrict__ qual) {
    const uint64_t i = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= n_slots) return;
    const uint8_t letter = letters[i];
    if (letter && place[i] < n_letters) {
        out[place[i]] = letter;
        if (QUAL) qual[place[i]] = (uint8_t)(33u + min(((uint32_t)slots[i] >> 8) & 0xFFu, ST_MAX_QUALITY));
    }
}

// where every piece's slots and letters begin (pieces lie one after the other in both)
__global__ void k_stitch_bounds(const uint64_t* __restrict__ pbase, int n_pieces, const uint32_t* __restrict__ slot_base,
                                const uint32_t* __restrict__ place, uint64_t n_positions, uint64_t n_slots, uint64_t n_letters,
                                uint64_t* __restrict__ letter_start) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pieces) return;
    const uint64_t at = pbase[p];
    const uint64_t slot = at < n_positions ? slot_base[at] : n_slots;
    letter_start[p] = slot < n_slots ? place[slot] : n_letters;
}

// ---------------------------------------------------------------- exclusive scan: scan.h ----
struct LoadLetter {
    const uint8_t* p;
    PA_DEV uint64_t operator()(uint64_t i) const { return p[i] != 0; }
};
// low word: the position has no slot; high word: ... and the position in front of it has one, so a run begins here.  Scanned
// into 32-bit outputs the low word alone survives; the 64-bit total carries both counts (each below 2^32: so are the positions).
struct LoadHole {
    const uint32_t* width;
    PA_DEV uint64_t operator()(uint64_t i) const {
        if (width[i] != 0) return 0;
        return 1ull | ((uint64_t)(i > 0 && width[i - 1] != 0) << 32);
    }
};

// ---------------------------------------------------------------- fill: the draft where no slot is ----
// One lane per position of the one piece.  holes[p]: positions without a slot in front of p; draft: the draft from the piece's
// first position on; lead: letters in front of the piece.  Consecutive lanes write consecutive letters wherever the widths are 1.
// A position with many insert slots is walked by its one lane (at most 65 536 slots; the edit passes deal a lane per slot
// because they bisect anyway, here the position's own tables give every address and a second bisection would cost every lane).
template <bool QUAL>
__global__ __launch_bounds__(ST_THREADS) void k_stitch_fill(const uint32_t* __restrict__ width, const uint32_t* __restrict__ slot_base,
                                                            const uint32_t* __restrict__ holes, const uint8_t* __restrict__ letters,
                                                            const uint32_t* __restrict__ place,
                                                            const unsigned long long* __restrict__ slots,
                                                            const uint8_t* __restrict__ draft, uint64_t n_positions, uint64_t n_slots,
                                                            uint64_t n_letters, uint64_t lead, uint64_t n_out, uint8_t* __restrict__ out,
                                                            uint8_t* __restrict__ qual) {
    const uint64_t p = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (p >= n_positions) return;
    const uint32_t w = width[p];
    const uint64_t base = slot_base[p], shift = lead + holes[p];
    if (w == 0) {                                        // (shares the base of the next position that has a slot)
        const uint64_t at = shift + (base < n_slots ? (uint64_t)place[base] : n_letters);
        if (at < n_out) {
            out[at] = draft[p];
            if (QUAL) qual[at] = (uint8_t)'!';
        }
        return;
    }
    for (uint64_t i = base; i < base + w && i < n_slots; ++i) {
        const uint8_t letter = letters[i];
        const uint64_t at = shift + place[i];
        if (letter && at < n_out) {
            out[at] = letter;
            if (QUAL) qual[at] = (uint8_t)(33u + min(((uint32_t)slots[i] >> 8) & 0xFFu, ST_MAX_QUALITY));
        }
    }
}

// ---------------------------------------------------------------- edits against the draft ----
struct EditTables {                                     // the last finish's tables, as the edit passes read them
    const uint32_t* slot_base;                          // [n_positions] slot of key (position, 0)
    const uint32_t* width;                              // [n_positions]
    const unsigned long long* slots;                    // [n_slots] winner words
    const uint8_t* letters;                             // [n_slots]
    const uint32_t* place;                              // [n_slots] letters in front of the slot, in table order
    const uint64_t* pbase;                              // [n_pieces] first position row of a piece
    const uint32_t* pmin;                               // [n_pieces] its first position
    const int64_t* letter_shift;                        // [n_pieces] take() offset of the piece's first letter - its table offset
    const uint16_t* take_index;                         // [n_pieces] the piece's place in take() order
    const uint8_t* draft;                               // draft[draft_lo .. draft_lo + draft_span)
    const uint32_t* holes;                              // [n_positions] after a fill: positions without a slot in front (else null)
    uint64_t n_positions, n_slots;
    uint32_t n_pieces, draft_lo, draft_span, qualities;
    uint32_t lead;                                      // after a fill: letters in front of the piece
};

struct SlotEdit {
    uint32_t kind;                                      // 0: none, else PA_EDIT_SUB / DEL / INS
    bool gap;                                           // the slot closes a run of uncovered positions
    uint32_t position, index, piece, open_at;           // open_at: first position of that run
    uint8_t draft, letter;
};

// the last i in [0, n) with v[i] <= key (v ascending, v[0] <= key)
template <class T, class K> PA_DEV uint64_t last_at_most(const T* __restrict__ v, uint64_t n, K key) {
    uint64_t lo = 0, hi = n;                             // v[lo] <= key < v[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (v[mid] <= key) lo = mid;
        else hi = mid;
    }
    return lo;
}

// letter: what the slot emits (the edit passes read letters[s]; the gate passes decode the winner word, which still holds the
// model's label while letters[] is being rewritten); RUNS: also look for the run of uncovered positions the slot closes
template <bool RUNS> PA_DEV SlotEdit classify_slot(const EditTables& t, uint64_t s, uint8_t letter) {
    SlotEdit e;
    // zero-width positions share the base of the next covered one: the LAST position whose base is <= s owns the slot
    const uint64_t gp = last_at_most(t.slot_base, t.n_positions, (uint32_t)s);
    e.piece = (uint32_t)last_at_most(t.pbase, (uint64_t)t.n_pieces, gp);      // (a piece without rows shares the next one's base)
    const uint64_t row0 = t.pbase[e.piece];
    e.position = t.pmin[e.piece] + (uint32_t)(gp - row0);
    e.index = (uint32_t)s - t.slot_base[gp];
    e.letter = letter;
    e.draft = 0;
    e.kind = 0;
    e.gap = false;
    e.open_at = 0;
    if (e.index > 0) {
        if (e.letter) e.kind = PA_EDIT_INS;
        return e;
    }
    const uint32_t at = e.position - t.draft_lo;
    uint8_t d = at < t.draft_span ? t.draft[at] : (uint8_t)0;
    if (d >= 'a' && d <= 'z') d = (uint8_t)(d - 32);
    e.draft = d;
    if (!e.letter) e.kind = PA_EDIT_DEL;
    else if (e.letter != d) e.kind = PA_EDIT_SUB;
    if (RUNS && gp > row0 && t.width[gp - 1] == 0) {    // the piece's first position has a slot, so slot s - 1 is the piece's too
        const uint64_t before = last_at_most(t.slot_base, t.n_positions, (uint32_t)(s - 1));
        e.gap = true;
        e.open_at = e.position - (uint32_t)(gp - before) + 1;
    }
    return e;
}

PA_DEV pa_stitch_edit make_edit(uint32_t position, uint32_t offset, uint32_t index, uint32_t piece, uint32_t kind, uint8_t draft,
                                uint8_t letter, uint8_t phred) {
    pa_stitch_edit r;
    r.position = position;
    r.offset = offset;
    r.index = (uint16_t)index;
    r.piece = (uint16_t)piece;
    r.kind = (uint8_t)kind;
    r.draft = draft;
    r.letter = letter;
    r.phred = phred;
    return r;
}

PA_DEV uint8_t word_letter(unsigned long long word) {
    const uint32_t label = (uint32_t)word & 0xFFu;
    return label >= 1 && label <= 4 ? (uint8_t)((0x54474341u >> (8 * (label - 1))) & 0xFFu) : (uint8_t)0;
}
PA_DEV uint32_t base_code(uint8_t d) { return d == 'A' ? 1u : d == 'C' ? 2u : d == 'G' ? 3u : d == 'T' ? 4u : 0u; }

// ---------------------------------------------------------------- the record passes: a rule, a count pass, a write pass ----
// A rule says what one slot yields -- slot(): a SlotEdit whose kind is 0 where the slot has no record of its own -- how many
// records that is, and what the slot's lane does beside the counting (counted) and beside the writing (written: only for a slot
// with a record of its own).  The two passes below do everything else, once.

// the edits of the consensus against the draft: 0 or 1 record per slot, and in front of it the GAP pair of the run it closes
struct EditRule {
    PA_DEV SlotEdit slot(const EditTables& t, uint64_t s) const { return classify_slot<true>(t, s, t.letters[s]); }
    PA_DEV static uint32_t records(const SlotEdit& e) { return (e.kind != 0) + (e.gap ? 2u : 0u); }
    PA_DEV void counted(uint64_t, const SlotEdit&) const {}
    // the run's two records go to out[run], out[run + 1]; letters_before: of the closing slot
    PA_DEV uint32_t write_run(const EditTables& t, const SlotEdit& e, uint32_t letters_before, uint32_t piece, uint64_t run,
                              uint64_t n_records, pa_stitch_edit* __restrict__ out) const {
        if (!e.gap) return 0;
        const uint32_t close_at = e.position - 1;
        const uint32_t lo = e.open_at - t.draft_lo, hi = close_at - t.draft_lo;
        uint8_t d_open = lo < t.draft_span ? t.draft[lo] : (uint8_t)0, d_close = hi < t.draft_span ? t.draft[hi] : (uint8_t)0;
        if (d_open >= 'a' && d_open <= 'z') d_open = (uint8_t)(d_open - 32);
        if (d_close >= 'a' && d_close <= 'z') d_close = (uint8_t)(d_close - 32);
        // after a fill the run's own letters are in the consensus, behind the pair's offset
        const uint32_t run_at = t.holes ? letters_before - (close_at - e.open_at + 1) : letters_before;
        if (run < n_records) out[run] = make_edit(e.open_at, run_at, 0, piece, PA_EDIT_GAP_OPEN, d_open, 0, 0);
        if (run + 1 < n_records) out[run + 1] = make_edit(close_at, run_at, 0, piece, PA_EDIT_GAP_CLOSE, d_close, 0, 0);
        return 2;
    }
    PA_DEV void written(uint64_t, const SlotEdit&) const {}
};

// the gate: the edit the winner makes against the draft where it is WITHHELD -- its phred is below min_phred; a SUB or DEL only
// where the draft letter is a base (the gate has no letter to keep elsewhere, and the model's decision stands).  Read off the
// winner word the finish left (the model's label and raw phred), not letters[]: the count pass rewrites letters[] while the write
// pass still has to find the model's letter.  A lane touches only its own slot.
struct GateRule {
    uint32_t min_phred;
    uint8_t* letters;                                   // count pass: a withheld slot's letter becomes what it emits now
    unsigned long long* slots;                          // write pass: its winner word loses its phred and takes that letter's label,
                                                        // so that emit, fill and edits read tables that agree with letters[]
    PA_DEV SlotEdit slot(const EditTables& t, uint64_t s) const {
        const unsigned long long word = t.slots[s];
        SlotEdit e = classify_slot<false>(t, s, word_letter(word));
        const uint32_t phred = (uint32_t)(word >> 8) & 0xFFu;      // (0: no writer)
        if (!(phred < min_phred && (e.kind == PA_EDIT_INS || base_code(e.draft) != 0))) e.kind = 0;
        return e;
    }
    PA_DEV static uint32_t records(const SlotEdit& e) { return e.kind != 0; }
    // what a withheld slot emits: the draft letter, nothing (0) for an INS
    PA_DEV static uint8_t emits(const SlotEdit& e) { return e.kind == PA_EDIT_INS ? (uint8_t)0 : e.draft; }
    PA_DEV void counted(uint64_t s, const SlotEdit& e) const {
        if (e.kind) letters[s] = emits(e);
    }
    PA_DEV uint32_t write_run(const EditTables&, const SlotEdit&, uint32_t, uint32_t, uint64_t, uint64_t, pa_stitch_edit*) const { return 0; }
    PA_DEV void written(uint64_t s, const SlotEdit& e) const { slots[s] = (slots[s] & ~0xFFFFull) | base_code(emits(e)); }
};

// count pass: sums[b] = records of slots [b * B, (b + 1) * B) (a workgroup past the end writes 0); kinds[k] += records of kind k
template <class Rule>
__global__ __launch_bounds__(ST_THREADS) void k_record_count(EditTables t, Rule rule, uint64_t* __restrict__ sums,
                                                             unsigned long long* __restrict__ kinds) {
    __shared__ uint64_t s_wave[ST_THREADS / 64];
    __shared__ uint64_t s_kind[ST_THREADS / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * ST_B + (uint64_t)threadIdx.x * ST_ITEMS;
    uint64_t v = 0, packed = 0;                         // packed: SUB | DEL << 16 | INS << 32 | gaps << 48 (a workgroup has <= 1024 each)
    for (int k = 0; k < ST_ITEMS; ++k) {
        if (i0 + k >= t.n_slots) break;
        const SlotEdit e = rule.slot(t, i0 + k);
        rule.counted(i0 + k, e);
        v += Rule::records(e);
        if (e.kind) packed += 1ull << (16 * (e.kind - 1));
        if (e.gap) packed += 1ull << 48;
    }
    for (int d = 32; d; d >>= 1)
        packed += ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(packed >> 32), d) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)packed, d);
    if ((threadIdx.x & 63) == 0) s_kind[threadIdx.x >> 6] = packed;
    uint64_t total;
    (void)block_scan(v, s_wave, &total);               // (its barrier also publishes s_kind)
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = total;
        uint64_t all = 0;
        for (int w = 0; w < ST_THREADS / 64; ++w) all += s_kind[w];
        const unsigned long long sub = all & 0xFFFFu, del = (all >> 16) & 0xFFFFu, ins = (all >> 32) & 0xFFFFu, gaps = all >> 48;
        if (sub) atomicAdd(&kinds[PA_EDIT_SUB], sub);     // one atomic per workgroup and kind; integer sums do not depend on the order
        if (del) atomicAdd(&kinds[PA_EDIT_DEL], del);
        if (ins) atomicAdd(&kinds[PA_EDIT_INS], ins);
        if (gaps) {
            atomicAdd(&kinds[PA_EDIT_GAP_OPEN], gaps);
            atomicAdd(&kinds[PA_EDIT_GAP_CLOSE], gaps);
        }
    }
}

// write pass (the gate's: after the letters were scanned again, t.place is the gated place): the records of slot i go to
// out[offset[b] + records of the block's slots in front of i ..): k_scan_down's walk with the rule in place of a load.
// piece_start[p] = where the records of piece p begin.
template <class Rule>
__global__ __launch_bounds__(ST_THREADS) void k_record_write(EditTables t, Rule rule, const uint64_t* __restrict__ offset,
                                                             uint64_t n_records, pa_stitch_edit* __restrict__ out,
                                                             uint64_t* __restrict__ piece_start) {
    __shared__ uint64_t s_wave[ST_THREADS / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * ST_B + (uint64_t)threadIdx.x * ST_ITEMS;
    SlotEdit item[ST_ITEMS];
    uint64_t v = 0;
    for (int k = 0; k < ST_ITEMS; ++k) {
        item[k].kind = 0;
        item[k].gap = false;
        if (i0 + k < t.n_slots) item[k] = rule.slot(t, i0 + k);
        v += Rule::records(item[k]);
    }
    uint64_t total;
    uint64_t run = block_scan(v, s_wave, &total) - v + offset[blockIdx.x];
    for (int k = 0; k < ST_ITEMS; ++k) {
        if (i0 + k >= t.n_slots) break;
        const SlotEdit& e = item[k];
        if (e.index == 0 && e.position == t.pmin[e.piece]) piece_start[e.piece] = run;
        if (Rule::records(e) == 0) continue;
        const uint32_t piece = t.take_index[e.piece];
        uint32_t letters_before = (uint32_t)((int64_t)t.place[i0 + k] + t.letter_shift[e.piece]);
        if (t.holes) letters_before += t.lead + t.holes[t.pbase[e.piece] + (e.position - t.pmin[e.piece])];      // (uniform)
        run += rule.write_run(t, e, letters_before, piece, run, n_records, out);
        if (e.kind) {
            const uint8_t phred = t.qualities ? (uint8_t)(((uint32_t)t.slots[i0 + k] >> 8) & 0xFFu) : (uint8_t)0;      // (the raw one)
            if (run < n_records)
                out[run] = make_edit(e.position, letters_before, e.index, piece, e.kind, e.draft, e.kind == PA_EDIT_DEL ? (uint8_t)0 : e.letter,
                                     phred);
            rule.written(i0 + k, e);
            run += 1;
        }
    }
}

// ---------------------------------------------------------------- gate: what it runs beside the record passes ----
// the withheld records of a gated finish that was filled afterwards: their offsets count the filled consensus, as the edit
// records' do (one piece: the row of a position is position - first)
__global__ void k_gate_filled_offsets(pa_stitch_edit* __restrict__ records, uint64_t n, const uint32_t* __restrict__ holes,
                                      uint64_t n_positions, uint32_t first, uint32_t lead) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t row = (uint64_t)(records[i].position - first);
    if (row < n_positions) records[i].offset += lead + holes[row];
}

// letter_shift[p] (take() offset of a piece's first letter - its table offset) of the gated pieces, before the host knows their
// lengths: the pieces with rows walked in take() order by one lane (a finish has a handful of pieces).  start[p] as
// k_stitch_bounds left it, ST_AT_END where a piece has no slot behind it.
constexpr uint64_t ST_AT_END = ~0ull;
__global__ void k_gate_shift(const uint16_t* __restrict__ order, uint32_t n_taken, const uint64_t* __restrict__ start, uint32_t n_pieces,
                             const uint64_t* __restrict__ n_letters, int64_t* __restrict__ shift) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t end = *n_letters;
    uint64_t at = 0;
    for (uint32_t k = 0; k < n_taken; ++k) {
        const uint32_t p = order[k];
        if (p >= n_pieces) continue;
        const uint64_t from = start[p] == ST_AT_END ? end : start[p];
        const uint64_t to = p + 1 < n_pieces && start[p + 1] != ST_AT_END ? start[p + 1] : end;
        shift[p] = (int64_t)at - (int64_t)from;
        at += to - from;
    }
}

// ---------------------------------------------------------------- variants: the hunks of the filled consensus, normalised ----
// (the rule: include/pepper_amd_encoder.h at pa_stitcher_variants; pepper_amd/polish/Variants.py records_numpy is the twin)
struct VarTables {
    const pa_stitch_edit* records;                      // of the filled consensus: one piece, keys in order
    const uint8_t* draft;                               // the whole contig as stored (compared upper-cased)
    const uint8_t* cons;                                // the filled consensus
    uint64_t n_records, draft_length, cons_length;
};

struct HunkWork {                                       // one hunk between the passes
    uint32_t first, last;                               // its records
    uint32_t q;                                         // the minimum of their phred
    uint32_t a, b, s, t;                                // trimmed: draft [a, b), consensus [s, t)
    uint32_t b0;                                        // the untrimmed end of its draft interval
};

PA_DEV uint8_t upper_letter(uint8_t c) { return c >= 'a' && c <= 'z' ? (uint8_t)(c - 32) : c; }
PA_DEV bool is_edit(const pa_stitch_edit& r) { return r.kind >= PA_EDIT_SUB && r.kind <= PA_EDIT_INS; }
PA_DEV uint32_t edit_d0(const pa_stitch_edit& r) { return r.position + (r.kind == PA_EDIT_INS); }
PA_DEV uint32_t edit_o1(const pa_stitch_edit& r) { return r.offset + (r.kind == PA_EDIT_SUB || r.kind == PA_EDIT_INS); }
// record i begins a hunk: an edit that does not continue the record in front of it in both coordinate systems
PA_DEV bool hunk_head(const pa_stitch_edit* __restrict__ rec, uint64_t i) {
    const pa_stitch_edit r = rec[i];
    if (!is_edit(r)) return false;
    if (i == 0) return true;
    const pa_stitch_edit q = rec[i - 1];
    return !(is_edit(q) && edit_d0(r) == q.position + 1 && r.offset == edit_o1(q));
}
struct LoadHead {
    const pa_stitch_edit* rec;
    PA_DEV uint64_t operator()(uint64_t i) const { return hunk_head(rec, i); }
};

// One lane per record.  before[i] = hunk heads in front of record i (the scan), so an edit lies in hunk before[i] + head - 1;
// the head and the last record of a hunk write its range, every record lowers its phred (an integer minimum: order-free).
__global__ __launch_bounds__(ST_THREADS) void k_var_ranges(const pa_stitch_edit* __restrict__ rec, uint64_t n,
                                                           const uint32_t* __restrict__ before, HunkWork* __restrict__ hunks,
                                                           uint64_t n_hunks) {
    const uint64_t i = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= n) return;
    const pa_stitch_edit r = rec[i];
    if (!is_edit(r)) return;
    const bool head = hunk_head(rec, i);
    const uint64_t h = (uint64_t)before[i] + (head ? 1 : 0) - 1;      // (the first edit is a head: never before[i] = 0 without one)
    if (h >= n_hunks) return;
    if (head) hunks[h].first = (uint32_t)i;
    if (i + 1 == n || !is_edit(rec[i + 1]) || hunk_head(rec, i + 1)) hunks[h].last = (uint32_t)i;
    atomicMin(&hunks[h].q, (uint32_t)r.phred);
}

// One lane per hunk: step 1 of the rule.  The loops are as long as the letters a complex hunk shares with the draft at its ends
// (a hunk is a handful of records; the long walk, the left-alignment, has a wave per hunk below).
__global__ __launch_bounds__(ST_THREADS) void k_var_trim(VarTables t, HunkWork* __restrict__ hunks, uint64_t n_hunks) {
    const uint64_t h = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (h >= n_hunks) return;
    HunkWork w = hunks[h];
    if (w.first >= t.n_records || w.last >= t.n_records) return;
    const pa_stitch_edit f = t.records[w.first], l = t.records[w.last];
    uint32_t a = edit_d0(f), b = l.position + 1, s = f.offset, e = edit_o1(l);
    w.b0 = b;
    while (b > a && e > s && b <= t.draft_length && e <= t.cons_length && upper_letter(t.draft[b - 1]) == t.cons[e - 1]) {
        --b;
        --e;
    }
    while (b > a && e > s && a < t.draft_length && s < t.cons_length && upper_letter(t.draft[a]) == t.cons[s]) {
        ++a;
        ++s;
    }
    w.a = a;
    w.b = b;
    w.s = s;
    w.t = e;
    hunks[h] = w;
}

PA_DEV bool pure_indel(const HunkWork& w) { return (w.b == w.a) != (w.t == w.s); }

// One lane per hunk: step 3's F, the first hunk that is not linked to the contig's start (an integer minimum: order-free)
__global__ __launch_bounds__(ST_THREADS) void k_var_link(const HunkWork* __restrict__ hunks, uint64_t n_hunks, uint32_t* __restrict__ first_unlinked) {
    const uint64_t h = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (h >= n_hunks) return;
    const HunkWork w = hunks[h];
    const bool link = pure_indel(w) && w.a == (h == 0 ? 0u : hunks[h - 1].b + 1u);
    if (!link) atomicMin(first_unlinked, (uint32_t)h);
}

// One WAVE per hunk: steps 2 and 3.  A pure indel of n letters moves left while V[x] == V[x + n] for x = a - 1, a - 2, ... down
// to bound + 1, V the draft (deletion) or draft[0, a) + alt (insertion): lane l compares place k + l + 1, a ballot finds the
// first mismatch, 64 places per step; consecutive lanes read consecutive bytes.  Lane 0 writes the record of hunk h to tmp[h]
// and whether it is one to emit[h]; the counts go through the workgroup's LDS, one atomic per workgroup and count (integer sums).
__global__ __launch_bounds__(ST_THREADS) void k_var_align(VarTables t, const HunkWork* __restrict__ hunks, uint64_t n_hunks,
                                                          const uint32_t* __restrict__ first_unlinked, uint32_t qualities,
                                                          pa_stitch_variant* __restrict__ tmp, uint8_t* __restrict__ emit,
                                                          unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long s_count[4];           // no-ops, unanchored, moved, places moved
    if (threadIdx.x < 4) s_count[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t h = (uint64_t)blockIdx.x * (ST_THREADS / 64) + (threadIdx.x >> 6);
    if (h < n_hunks) {                                   // (uniform for the wave)
        const HunkWork w = hunks[h];
        const uint64_t F = *first_unlinked;
        const uint32_t rn = w.b - w.a, an = w.t - w.s;
        uint32_t position = w.a, ref_len = rn, alt_len = an, lead = 0, k = 0, kind = rn == an ? PA_VARIANT_SUB : PA_VARIANT_COMPLEX;
        bool keep = true, tail = false, noop = false, unanchored = false;
        if (rn == 0 && an == 0) {
            keep = false;
            noop = true;
        } else if (rn == 0 || an == 0) {
            const bool del = rn > 0;
            kind = del ? PA_VARIANT_DEL : PA_VARIANT_INS;
            ref_len = rn + 1;
            alt_len = an + 1;
            if (h < F) {                                 // anchored on the right
                tail = true;
                if (w.b >= t.draft_length) {
                    keep = false;
                    unanchored = true;
                }
            } else {
                const uint32_t bound = h == 0 ? 0u : h == F ? hunks[h - 1].b + 1u : hunks[h - 1].b0;
                const uint32_t n = del ? rn : an;
                const uint32_t room = w.a > bound ? w.a - 1u - bound : 0u;      // places it may move at most (a - 1 >= bound by the rule)
                while (k < room) {
                    const uint32_t j = k + lane + 1;
                    bool same = false;
                    if (j <= room) {
                        const uint64_t x = w.a - j, y = x + n;
                        if (!del && y >= w.a) {
                            const uint64_t c = (uint64_t)w.s + (y - w.a);
                            same = x < t.draft_length && c < t.cons_length && upper_letter(t.draft[x]) == t.cons[c];
                        } else {
                            same = y < t.draft_length && upper_letter(t.draft[x]) == upper_letter(t.draft[y]);
                        }
                    }
                    const unsigned long long miss = __ballot(!same);
                    if (miss) {
                        k += (uint32_t)__ffsll((long long)miss) - 1u;
                        break;
                    }
                    k += 64;
                }
                position = w.a - k - 1u;
                lead = del ? 1u : 1u + min(k, an);
            }
        }
        if (lane == 0) {
            pa_stitch_variant v;
            v.position = position;
            v.ref_len = ref_len;
            v.alt_len = alt_len;
            v.lead = lead;
            v.offset = w.s;
            v.shift = k;
            v.phred = qualities ? (uint8_t)min(w.q, 255u) : (uint8_t)0;
            v.kind = (uint8_t)kind;
            v.tail = tail ? 1 : 0;
            v.pad = 0;
            v.reserved = 0;
            tmp[h] = v;
            emit[h] = keep ? 1 : 0;
            if (noop) atomicAdd(&s_count[0], 1ull);
            if (unanchored) atomicAdd(&s_count[1], 1ull);
            if (k) {
                atomicAdd(&s_count[2], 1ull);
                atomicAdd(&s_count[3], (unsigned long long)k);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_count[threadIdx.x]) atomicAdd(&counts[1 + threadIdx.x], s_count[threadIdx.x]);
}

// the records that are ones, in hunk order: place[h] = records in front of hunk h (the scan of emit)
__global__ __launch_bounds__(ST_THREADS) void k_var_compact(const pa_stitch_variant* __restrict__ tmp, const uint8_t* __restrict__ emit,
                                                            const uint32_t* __restrict__ place, uint64_t n_hunks, uint64_t n_out,
                                                            pa_stitch_variant* __restrict__ out) {
    const uint64_t h = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (h >= n_hunks || !emit[h]) return;
    if (place[h] < n_out) out[place[h]] = tmp[h];
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
    Buffer() = default;
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    ~Buffer() {                                         // (with the handle: pa_stitcher_destroy has set the device and waited)
        if (p) (void)hipFree(p);
    }
    template <class T> T* as() const { return (T*)p; }
};

// The finish's piece words (f_piece): [pmin u32 | pmax u32 | pbase u64 | letter_start u64] x n_pieces, then fault, bad label
struct PieceWords {
    uint8_t* base;
    size_t np;
    static size_t at_pbase(size_t np) { return (np * 8 + 7) / 8 * 8; }
    static size_t bytes(size_t np) { return at_pbase(np) + np * 16 + 16; }
    uint32_t* pmin() const { return (uint32_t*)base; }
    uint32_t* pmax() const { return (uint32_t*)(base + np * 4); }
    uint64_t* pbase() const { return (uint64_t*)(base + at_pbase(np)); }
    uint64_t* letter_start() const { return pbase() + np; }
    uint32_t* flags() const { return (uint32_t*)(letter_start() + np); }      // [2]: a row outside its tables, the largest bad label
};

// The record passes' per-piece block (e_piece, g_piece): what the host says per piece (table order) -- what turns a table letter
// offset into a take() offset, its place in take() order -- and the device's answers: where a piece's records begin, the records
// per kind.  [letter_shift i64 | start u64] x n_pieces, kinds u64 x 6, [take_index u16 | order u16] x n_pieces
struct RecordWords {
    uint8_t* base;
    size_t np;
    static size_t bytes(size_t np) { return np * 20 + 6 * 8; }
    int64_t* letter_shift() const { return (int64_t*)base; }
    uint64_t* start() const { return (uint64_t*)base + np; }
    unsigned long long* kinds() const { return (unsigned long long*)(start() + np); }
    uint16_t* take_index() const { return (uint16_t*)(kinds() + 6); }
    uint16_t* order() const { return take_index() + np; }      // the gate's: the pieces with rows as take() goes
    // what a caller zeroes in one piece: start and kinds; with letter_shift in front of them where the device writes that too
    size_t answer_bytes() const { return np * 8 + 6 * 8; }
    size_t device_bytes() const { return np * 8 + answer_bytes(); }
};

struct ChunkRec {
    int32_t region;
    int64_t order;
    uint64_t arrival;
    uint64_t* rows;
    uint32_t count;
    bool qualities;                                     // added through pa_stitcher_add_qual: its rows carry their phred
};

struct PieceOut {
    int64_t first, last, offset, length;
    int piece;
};

// What the calls behind a finish make of its tables.  A product is live from the call that made it until a call that drops it.
enum Product { EDITS, FILL, WITHHELD, VARIANTS, N_PRODUCTS };
struct ProductState {
    bool live = false;
    int64_t count = 0;                                  // its records (FILL: its letters)
    int64_t bytes = 0;                                  // its share of the table bytes pa_stitcher_stats reports
};
// The one invalidation rule: what a call drops when it starts its work (its own product, to be made anew, among them).  A gate
// changes the consensus the edits describe; a fill changes it again, and the variants are the filled consensus' own; the withheld
// records outlive a fill (their offsets are moved once: withheld_filled).
enum Call { CALL_FINISH, CALL_GATE, CALL_FILL, CALL_EDITS, CALL_VARIANTS };
constexpr unsigned DROPS[] = {
    /* finish   */ 1u << EDITS | 1u << FILL | 1u << WITHHELD | 1u << VARIANTS,
    /* gate     */ 1u << EDITS,
    /* fill     */ 1u << EDITS | 1u << FILL | 1u << VARIANTS,
    /* edits    */ 1u << EDITS,
    /* variants */ 1u << VARIANTS,
};

}  // namespace

struct pa_stitcher {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::mutex lock;
    std::vector<uint64_t*> slabs;
    size_t slab_at = 0;                                 // slabs in use: the last of them is being filled
    int64_t slab_used = ST_SLAB_ROWS;                   // rows taken of it (no slab yet: "full")
    std::unordered_map<int32_t, std::vector<ChunkRec>> contigs;
    uint64_t arrivals = 0;
    int64_t rows_held = 0;
    // add's staging
    Buffer a_pos, a_idx, a_lab, a_phr, a_drop, a_kept, a_refused, a_dst;
    // finish's tables (f_qual: only once a contig came with qualities)
    Buffer f_desc, f_piece, f_width, f_base, f_slots, f_letters, f_place, f_out, f_qual, f_scan, f_words;
    // edits' staging (the draft span, the pieces' take() order) and its one table: the records
    Buffer e_draft, e_piece, e_records;
    // fill's tables: the positions without a slot in front of every position, the filled sequence, the filled qualities
    Buffer f_holes, f_fill, f_fillq;
    // gate's staging (per piece: letter shift, where its records begin, its take() place; the counts) and the withheld records
    Buffer g_piece, g_records;
    // variants' tables: hunk heads in front of every edit record, the hunks, their records before and after the compaction, the
    // flags and places of the compaction, scan scratch, the counts
    Buffer v_before, v_hunks, v_tmp, v_emit, v_place, v_out, v_scan, v_words;
    // what is live since the last finish.  EDITS: pa_stitcher_edits ran on the tables as they are.  FILL: pa_stitcher_fill ran --
    // take, take_qualities, edits speak of the filled consensus.  WITHHELD: pa_stitcher_gate ran -- every later call speaks of the
    // gated tables.  VARIANTS: pa_stitcher_variants ran on that fill.
    ProductState product[N_PRODUCTS];
    int64_t fill_lead = 0;                              // of the live fill: letters in front of the piece
    int64_t fill_draft_length = -1;                     // ... and the draft_length it was given
    bool withheld_filled = false;                       // the withheld records' offsets already count the fill that followed
    int64_t draft_held = -1;                            // e_draft holds draft[0 .. draft_held) of a fill, gate or variants (-1: it does not)
    std::vector<PieceOut> pieces;                      // of the last finish, in output order
    int64_t sequence_length = 0;
    bool finished = false;                              // a finish has run: the three below speak of it
    bool contig_qualities = false;                      // every chunk of its contig came with qualities
    bool have_qualities = false;                        // ... and it got as far as the emit: f_qual holds them
    int64_t last_slots = 0, last_pieces = 0, last_positions = 0;
    int64_t base_bytes = 0;                             // the finish's own table bytes (a gate moves them by the letters it moves)
    bool have_sequence = false;                         // the last finish ran to its end: its tables are whole

    bool live(Product p) const { return product[p].live; }
    void make(Product p, int64_t count, int64_t bytes) { product[p] = ProductState{true, count, bytes}; }
    void drop(Product p) {
        product[p] = ProductState();
        if (p == FILL) {
            fill_lead = 0;
            fill_draft_length = -1;
        }
        if (p == WITHHELD) withheld_filled = false;
    }
    void begin(Call call) {
        for (int p = 0; p < N_PRODUCTS; ++p)
            if (DROPS[call] >> p & 1u) drop((Product)p);
    }
    int64_t table_bytes() const {
        int64_t bytes = base_bytes;
        for (const ProductState& p : product) bytes += p.bytes;      // (a dropped product has none)
        return bytes;
    }
};

namespace {

#define ST_HIP(expr)                                                                                                 \
    do {                                                                                                             \
        hipError_t e_ = (expr);                                                                                      \
        if (e_ != hipSuccess) return pa::set_error(PA_ERR_HIP, std::string("stitcher: " #expr ": ") + hipGetErrorString(e_)); \
    } while (0)

int no_memory(const char* what, uint64_t bytes) {
    (void)hipGetLastError();
    return pa::set_error(PA_ERR_HIP, std::string("stitcher: no device memory for ") + what + " (" + std::to_string(bytes) + " bytes)");
}

// the refusals of every call that reads the last finish's tables, in the caller's name (whole: they are there to be read)
int needs_finish(const pa_stitcher* s, const char* who, bool whole) {
    if (!s->finished) return pa::set_error(PA_ERR_INVALID, std::string(who) + ": no contig has been finished");
    if (!whole) return pa::set_error(PA_ERR_INVALID, std::string(who) + ": the last finish gave no sequence (a label that is no base, or it failed)");
    return PA_OK;
}

// kernel<true> where there is a `qual` to write, else kernel<false>; `qual` is the kernels' last argument
template <class Kernel, class... Args>
void launch_qual(Kernel with, Kernel without, unsigned blocks, hipStream_t stream, uint8_t* qual, Args... args) {
    (qual ? with : without)<<<blocks, ST_THREADS, 0, stream>>>(args..., qual);
}

// pa_stitcher_take / pa_stitcher_take_qualities: the filled buffer as it lies, else the pieces in order
int take_letters(pa_stitcher* s, const Buffer& filled, const Buffer& pieces, char* dst, int64_t capacity, const char* who) {
    const int64_t length = s->live(FILL) ? s->product[FILL].count : s->sequence_length;
    if (capacity < length)
        return pa::set_error(PA_ERR_INVALID, std::string(who) + ": the sequence has " + std::to_string(length) + " letters, room for " +
                                                 std::to_string(capacity));
    ST_HIP(hipSetDevice(s->device));
    if (s->live(FILL)) {
        if (length > 0) ST_HIP(hipMemcpyAsync(dst, filled.p, (size_t)length, hipMemcpyDeviceToHost, s->stream));
        ST_HIP(hipStreamSynchronize(s->stream));
        return PA_OK;
    }
    int64_t at = 0;
    for (const PieceOut& piece : s->pieces) {
        if (piece.length == 0) continue;
        ST_HIP(hipMemcpyAsync(dst + at, pieces.as<uint8_t>() + piece.offset, (size_t)piece.length, hipMemcpyDeviceToHost, s->stream));
        at += piece.length;
    }
    ST_HIP(hipStreamSynchronize(s->stream));
    return PA_OK;
}

// The last finish's tables as the record passes read them, with the per-piece block `w`; the draft window (none), the fill's holes
// and lead (none) are the caller's to set
EditTables tables_of(const pa_stitcher* s, const RecordWords& w) {
    const PieceWords pw{s->f_piece.as<uint8_t>(), w.np};
    EditTables t;
    t.slot_base = s->f_base.as<uint32_t>();
    t.width = s->f_width.as<uint32_t>();
    t.slots = s->f_slots.as<unsigned long long>();
    t.letters = s->f_letters.as<uint8_t>();
    t.place = s->f_place.as<uint32_t>();
    t.pbase = pw.pbase();
    t.pmin = pw.pmin();
    t.letter_shift = w.letter_shift();
    t.take_index = w.take_index();
    t.draft = nullptr;
    t.holes = nullptr;
    t.n_positions = (uint64_t)s->last_positions;
    t.n_slots = (uint64_t)s->last_slots;
    t.n_pieces = (uint32_t)w.np;
    t.draft_lo = t.draft_span = t.lead = 0;
    t.qualities = s->contig_qualities ? 1u : 0u;
    return t;
}

// The count pass of `rule` into the block sums, the scan of the sums, and the total and the kinds read behind ONE wait.  `between`
// queues what the caller has to run behind the count pass and read behind the same wait.
template <class Rule, class Between>
int count_records(pa_stitcher* s, const EditTables& t, const Rule& rule, uint64_t* sums, unsigned long long* d_kinds, Between between,
                  uint64_t* total, uint64_t* kinds) {
    const uint64_t blocks = scan_blocks(t.n_slots);
    k_record_count<Rule><<<(unsigned)(blocks + 1), ST_THREADS, 0, s->stream>>>(t, rule, sums, d_kinds);
    ST_HIP(hipGetLastError());
    const int rc = between();
    if (rc != PA_OK) return rc;
    scan_sums(s->stream, sums, blocks + 1, sums + blocks + 1);
    ST_HIP(hipGetLastError());
    ST_HIP(hipMemcpyAsync(total, sums + blocks, 8, hipMemcpyDeviceToHost, s->stream));
    ST_HIP(hipMemcpyAsync(kinds, d_kinds, 6 * 8, hipMemcpyDeviceToHost, s->stream));
    ST_HIP(hipStreamSynchronize(s->stream));
    return PA_OK;
}

// Records the write passes left piece after piece in TABLE order (start[p]: where those of table piece p begin, on the device)
// -> dst, piece after piece as take() goes
int take_records(pa_stitcher* s, const uint64_t* d_start, const pa_stitch_edit* records, int64_t n, pa_stitch_edit* dst, const char* what) {
    const size_t np = (size_t)s->last_pieces;
    std::vector<uint64_t> start(np);
    ST_HIP(hipMemcpyAsync(start.data(), d_start, np * 8, hipMemcpyDeviceToHost, s->stream));
    ST_HIP(hipStreamSynchronize(s->stream));
    // in the buffer the pieces lie in table order: a piece's records end where those of the next piece with rows begin
    std::vector<std::pair<int, uint64_t>> table;
    for (const PieceOut& piece : s->pieces) table.push_back({piece.piece, start[(size_t)piece.piece]});
    std::sort(table.begin(), table.end());
    std::vector<uint64_t> end_of(np, 0);
    for (size_t k = 0; k < table.size(); ++k) end_of[(size_t)table[k].first] = k + 1 < table.size() ? table[k + 1].second : (uint64_t)n;
    int64_t at = 0;
    for (const PieceOut& piece : s->pieces) {
        const uint64_t begin = start[(size_t)piece.piece], end = end_of[(size_t)piece.piece];
        if (begin > end || end > (uint64_t)n || at + (int64_t)(end - begin) > n)
            return pa::set_error(PA_ERR_HIP, std::string(what) + ": a piece's records lie outside the buffer");
        if (end == begin) continue;
        ST_HIP(hipMemcpyAsync(dst + at, records + begin, (size_t)(end - begin) * sizeof(pa_stitch_edit), hipMemcpyDeviceToHost, s->stream));
        at += (int64_t)(end - begin);
    }
    ST_HIP(hipStreamSynchronize(s->stream));
    return PA_OK;
}

}  // namespace

extern "C" {

int pa_stitcher_limits(int64_t* out, int32_t n) {
    if (!out || n < 0) return pa::set_error(PA_ERR_INVALID, "stitcher limits: null or negative argument");
    const int64_t v[4] = {ST_MAX_POSITION, ST_MAX_INDEX, ST_B, ST_SLAB_ROWS};
    for (int32_t i = 0; i < n; ++i) out[i] = i < 4 ? v[i] : 0;
    return PA_OK;
}

int pa_stitcher_create(int32_t device, void* hip_stream, pa_stitcher** out) {
    if (!out) return pa::set_error(PA_ERR_INVALID, "stitcher: null argument");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return pa::set_error(PA_ERR_NO_DEVICE, "no HIP device visible: the device stitch has no CPU fallback (perform_stitch is the host form)");
    if (device < 0 || device >= count) return pa::set_error(PA_ERR_INVALID, "stitcher: device ordinal out of range");
    ST_HIP(hipSetDevice(device));
    auto* s = new pa_stitcher();
    s->device = device;
    s->stream = (hipStream_t)hip_stream;
    if (!hip_stream) {
        if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
            delete s;
            return pa::set_error(PA_ERR_HIP, "stitcher: stream creation failed");
        }
        s->own_stream = true;
    }
    *out = s;
    return PA_OK;
}

void pa_stitcher_destroy(pa_stitcher* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    for (uint64_t* slab : s->slabs) (void)hipFree(slab);
    if (s->own_stream) (void)hipStreamDestroy(s->stream);
    delete s;                                           // (its Buffers free themselves)
}

}  // extern "C"

namespace {

// pa_stitcher_add (with_phred false, phred unused) and pa_stitcher_add_qual
int stitcher_add(pa_stitcher* s, int32_t contig, int32_t n_chunks, int32_t chunk_len, const int64_t* position, const int64_t* index,
                 const uint8_t* labels, const uint8_t* phred, bool with_phred, int32_t labels_on_device, const int32_t* region,
                 const int64_t* chunk_order, const int64_t* drop_below) {
    if (!s || n_chunks < 0 || chunk_len < 0) return pa::set_error(PA_ERR_INVALID, "stitcher add: null handle or negative size");
    if (n_chunks == 0 || chunk_len == 0) return PA_OK;
    if (!position || !index || !labels || (with_phred && !phred) || !region || !chunk_order || !drop_below)
        return pa::set_error(PA_ERR_INVALID, "stitcher add: null array");
    std::lock_guard<std::mutex> guard(s->lock);
    ST_HIP(hipSetDevice(s->device));
    const size_t n = (size_t)n_chunks, rows = n * (size_t)chunk_len;
    if (!s->a_pos.grow(rows * 8) || !s->a_idx.grow(rows * 8) || !s->a_drop.grow(n * 8) || !s->a_kept.grow(n * 4) ||
        !s->a_refused.grow(n * 4) || !s->a_dst.grow(n * 8) || (!labels_on_device && !s->a_lab.grow(rows)) ||
        (with_phred && !labels_on_device && !s->a_phr.grow(rows)))
        return no_memory("the staged chunks", rows * (with_phred ? 18 : 17));
    ST_HIP(hipMemcpyAsync(s->a_pos.p, position, rows * 8, hipMemcpyHostToDevice, s->stream));
    ST_HIP(hipMemcpyAsync(s->a_idx.p, index, rows * 8, hipMemcpyHostToDevice, s->stream));
    ST_HIP(hipMemcpyAsync(s->a_drop.p, drop_below, n * 8, hipMemcpyHostToDevice, s->stream));
    const uint8_t* d_labels = labels;
    if (!labels_on_device) {
        ST_HIP(hipMemcpyAsync(s->a_lab.p, labels, rows, hipMemcpyHostToDevice, s->stream));
        d_labels = s->a_lab.as<uint8_t>();
    }
    const uint8_t* d_phred = with_phred ? phred : nullptr;
    if (with_phred && !labels_on_device) {
        ST_HIP(hipMemcpyAsync(s->a_phr.p, phred, rows, hipMemcpyHostToDevice, s->stream));
        d_phred = s->a_phr.as<uint8_t>();
    }
    k_stitch_count<<<(unsigned)n, ST_THREADS, 0, s->stream>>>(s->a_pos.as<int64_t>(), s->a_idx.as<int64_t>(), s->a_drop.as<int64_t>(),
                                                               chunk_len, s->a_kept.as<int32_t>(), s->a_refused.as<int32_t>());
    ST_HIP(hipGetLastError());
    std::vector<int32_t> kept(n), refused(n);
    ST_HIP(hipMemcpyAsync(kept.data(), s->a_kept.p, n * 4, hipMemcpyDeviceToHost, s->stream));
    ST_HIP(hipMemcpyAsync(refused.data(), s->a_refused.p, n * 4, hipMemcpyDeviceToHost, s->stream));
    ST_HIP(hipStreamSynchronize(s->stream));
    for (size_t c = 0; c < n; ++c) {
        if (refused[c])
            return pa::set_error(PA_ERR_UNSUPPORTED, "stitcher add: chunk " + std::to_string(c) + " of the call holds a kept row with a position above " +
                                                         std::to_string(ST_MAX_POSITION) + " or an insert index above " +
                                                         std::to_string(ST_MAX_INDEX) + "; nothing of the call was taken");
        if (kept[c] > ST_SLAB_ROWS)
            return pa::set_error(PA_ERR_UNSUPPORTED, "stitcher add: chunk " + std::to_string(c) + " keeps " + std::to_string(kept[c]) +
                                                         " rows, a slab holds " + std::to_string(ST_SLAB_ROWS) + "; nothing of the call was taken");
    }
    // every chunk's place: behind the last one while the slab has room, else at the head of a new slab
    std::vector<uint64_t*> dst(n, nullptr);
    size_t slab = s->slab_at;
    int64_t used = s->slab_used;
    for (size_t c = 0; c < n; ++c) {
        if (kept[c] == 0) continue;
        if (used + kept[c] > ST_SLAB_ROWS) {
            if (slab == s->slabs.size()) {
                uint64_t* fresh = nullptr;
                if (hipMalloc((void**)&fresh, (size_t)ST_SLAB_ROWS * 8) != hipSuccess) return no_memory("a slab", (uint64_t)ST_SLAB_ROWS * 8);
                s->slabs.push_back(fresh);              // (kept if the call fails later: the cursor has not moved, the next call fills it)
            }
            ++slab;
            used = 0;
        }
        dst[c] = s->slabs[slab - 1] + used;
        used += kept[c];
    }
    ST_HIP(hipMemcpyAsync(s->a_dst.p, dst.data(), n * 8, hipMemcpyHostToDevice, s->stream));
    k_stitch_compact<<<(unsigned)n, ST_THREADS, 0, s->stream>>>(s->a_pos.as<int64_t>(), s->a_idx.as<int64_t>(), d_labels, d_phred,
                                                                 s->a_drop.as<int64_t>(), chunk_len, s->a_kept.as<int32_t>(),
                                                                 s->a_dst.as<uint64_t*>());
    ST_HIP(hipGetLastError());
    ST_HIP(hipStreamSynchronize(s->stream));            // the caller's arrays, labels and phred are free again; dst is read
    auto& list = s->contigs[contig];
    for (size_t c = 0; c < n; ++c) {
        if (kept[c] == 0) continue;
        list.push_back(ChunkRec{region[c], chunk_order[c], s->arrivals++, dst[c], (uint32_t)kept[c], with_phred});
        s->rows_held += kept[c];
    }
    s->slab_at = slab;
    s->slab_used = used;
    return PA_OK;
}

}  // namespace

extern "C" {

int pa_stitcher_add(pa_stitcher* s, int32_t contig, int32_t n_chunks, int32_t chunk_len, const int64_t* position, const int64_t* index,
                    const uint8_t* labels, int32_t labels_on_device, const int32_t* region, const int64_t* chunk_order,
                    const int64_t* drop_below) {
    return stitcher_add(s, contig, n_chunks, chunk_len, position, index, labels, nullptr, false, labels_on_device, region, chunk_order,
                        drop_below);
}

int pa_stitcher_add_qual(pa_stitcher* s, int32_t contig, int32_t n_chunks, int32_t chunk_len, const int64_t* position,
                         const int64_t* index, const uint8_t* labels, const uint8_t* phred, int32_t labels_on_device,
                         const int32_t* region, const int64_t* chunk_order, const int64_t* drop_below) {
    return stitcher_add(s, contig, n_chunks, chunk_len, position, index, labels, phred, true, labels_on_device, region, chunk_order,
                        drop_below);
}

int pa_stitcher_finish(pa_stitcher* s, int32_t contig, int32_t n_regions, const int32_t* region, const int32_t* piece, const int64_t* rank,
                       int32_t n_pieces, int64_t* piece_first, int64_t* piece_last, int64_t* piece_length, int64_t* sequence_length,
                       int32_t* bad_label) {
    if (!s || n_regions < 0 || n_pieces < 0 || !sequence_length || !bad_label ||
        (n_regions > 0 && (!region || !piece || !rank)) || (n_pieces > 0 && (!piece_first || !piece_last || !piece_length)))
        return pa::set_error(PA_ERR_INVALID, "stitcher finish: null or negative argument");
    std::lock_guard<std::mutex> guard(s->lock);
    ST_HIP(hipSetDevice(s->device));
    *sequence_length = 0;
    *bad_label = 0;
    s->pieces.clear();
    s->sequence_length = 0;
    s->finished = true;
    s->contig_qualities = s->have_qualities = false;
    s->have_sequence = false;
    s->begin(CALL_FINISH);
    s->draft_held = -1;
    s->last_slots = s->last_positions = s->base_bytes = 0;
    s->last_pieces = n_pieces;
    for (int32_t p = 0; p < n_pieces; ++p) {
        piece_first[p] = piece_last[p] = -1;
        piece_length[p] = 0;
    }
    std::unordered_map<int32_t, std::pair<int32_t, int64_t>> where;      // region id -> (piece, rank)
    for (int32_t r = 0; r < n_regions; ++r) {
        if (piece[r] < 0 || piece[r] >= n_pieces) return pa::set_error(PA_ERR_INVALID, "stitcher finish: a region's piece is out of range");
        where[region[r]] = {piece[r], rank[r]};
    }
    auto found = s->contigs.find(contig);
    if (found == s->contigs.end() || found->second.empty() || n_pieces == 0) {
        if (found != s->contigs.end() && !found->second.empty())
            return pa::set_error(PA_ERR_INVALID, "stitcher finish: the contig holds chunks and the plan has no piece");
        s->contig_qualities = s->have_qualities = true;  // no chunk came without them: the empty sequence has empty qualities
        s->have_sequence = true;
        return PA_OK;
    }
    // loop order: regions as ranked, a region's chunks by their order value, equal ones as they arrived
    struct Ordered { int64_t rank; const ChunkRec* rec; int32_t piece; };
    std::vector<Ordered> order;
    order.reserve(found->second.size());
    for (const ChunkRec& rec : found->second) {
        auto w = where.find(rec.region);
        if (w == where.end())
            return pa::set_error(PA_ERR_INVALID, "stitcher finish: region " + std::to_string(rec.region) + " holds chunks and is not in the plan");
        order.push_back(Ordered{w->second.second, &rec, w->second.first});
    }
    std::sort(order.begin(), order.end(), [](const Ordered& a, const Ordered& b) {
        if (a.rank != b.rank) return a.rank < b.rank;
        if (a.rec->order != b.rec->order) return a.rec->order < b.rec->order;
        return a.rec->arrival < b.rec->arrival;
    });
    const size_t n_desc = order.size();
    std::vector<ChunkDesc> desc(n_desc);
    std::vector<int64_t> piece_rows((size_t)n_pieces, 0);
    uint64_t rank_base = 0;
    bool qualities = true;                              // on when every chunk of the contig came with them
    for (size_t i = 0; i < n_desc; ++i) {
        desc[i] = ChunkDesc{order[i].rec->rows, order[i].rec->count, (uint32_t)order[i].piece, rank_base};
        rank_base += order[i].rec->count;
        piece_rows[(size_t)order[i].piece] += order[i].rec->count;
        qualities = qualities && order[i].rec->qualities;
    }
    if (rank_base > ST_MAX_ROWS)                        // (rank + 1 of the last row = rank_base)
        return pa::set_error(PA_ERR_UNSUPPORTED, "stitcher finish: the contig keeps " + std::to_string(rank_base) +
                                                     " rows, the scatter word ranks 2^48 - 1");
    s->contig_qualities = qualities;
    const size_t np = (size_t)n_pieces;
    if (!s->f_desc.grow(n_desc * sizeof(ChunkDesc)) || !s->f_piece.grow(PieceWords::bytes(np)))
        return no_memory("the chunk table", n_desc * sizeof(ChunkDesc));
    const PieceWords pw{s->f_piece.as<uint8_t>(), np};
    uint32_t *d_pmin = pw.pmin(), *d_pmax = pw.pmax(), *d_fault = pw.flags(), *d_bad = pw.flags() + 1;
    uint64_t *d_pbase = pw.pbase(), *d_start = pw.letter_start();
    ST_HIP(hipMemcpyAsync(s->f_desc.p, desc.data(), n_desc * sizeof(ChunkDesc), hipMemcpyHostToDevice, s->stream));
    ST_HIP(hipMemsetAsync(d_pmin, 0xFF, np * 4, s->stream));
    ST_HIP(hipMemsetAsync(d_pmax, 0, np * 4, s->stream));
    ST_HIP(hipMemsetAsync(d_fault, 0, 8, s->stream));
    // 1. range
    k_stitch_range<<<(unsigned)n_desc, ST_THREADS, 0, s->stream>>>(s->f_desc.as<ChunkDesc>(), d_pmin, d_pmax);
    ST_HIP(hipGetLastError());
    std::vector<uint32_t> pmin(np), pmax(np);
    ST_HIP(hipMemcpyAsync(pmin.data(), d_pmin, np * 4, hipMemcpyDeviceToHost, s->stream));
    ST_HIP(hipMemcpyAsync(pmax.data(), d_pmax, np * 4, hipMemcpyDeviceToHost, s->stream));
    ST_HIP(hipStreamSynchronize(s->stream));
    std::vector<uint64_t> pbase(np);
    uint64_t n_positions = 0;
    for (size_t p = 0; p < np; ++p) {
        pbase[p] = n_positions;
        if (piece_rows[p] > 0) {
            if (pmin[p] > pmax[p]) return pa::set_error(PA_ERR_HIP, "stitcher finish: a piece with rows has no position range");
            n_positions += (uint64_t)pmax[p] - pmin[p] + 1;
            piece_first[p] = pmin[p];
            piece_last[p] = pmax[p];
        }
    }
    s->last_positions = (int64_t)n_positions;
    // 2. widths, 3. their scan
    const uint64_t scan_words = std::max(scan_scratch_words(n_positions), (uint64_t)1);
    if (!s->f_width.grow(n_positions * 4) || !s->f_base.grow(n_positions * 4) || !s->f_scan.grow(scan_words * 8))
        return no_memory("the width table", n_positions * 8);
    ST_HIP(hipMemcpyAsync(d_pbase, pbase.data(), np * 8, hipMemcpyHostToDevice, s->stream));
    ST_HIP(hipMemsetAsync(s->f_width.p, 0, n_positions * 4, s->stream));
    k_stitch_width<<<(unsigned)n_desc, ST_THREADS, 0, s->stream>>>(s->f_desc.as<ChunkDesc>(), d_pmin, d_pbase, s->f_width.as<uint32_t>(),
                                                                    n_positions, d_fault);
    ST_HIP(hipGetLastError());
    const uint64_t* d_total = scan_exclusive<LoadU32, uint32_t>(s->stream, LoadU32{s->f_width.as<uint32_t>()}, n_positions,
                                                                s->f_base.as<uint32_t>(), s->f_scan.as<uint64_t>());
    ST_HIP(hipGetLastError());
    uint64_t n_slots = 0;
    ST_HIP(hipMemcpyAsync(&n_slots, d_total, 8, hipMemcpyDeviceToHost, s->stream));
    ST_HIP(hipStreamSynchronize(s->stream));
    if (n_slots > 0xFFFFFFFFull)
        return pa::set_error(PA_ERR_UNSUPPORTED, "stitcher finish: the contig needs " + std::to_string(n_slots) + " slots, the tables index 2^32 - 1");
    s->last_slots = (int64_t)n_slots;
    // 4. scatter, 5. check and count
    const uint64_t letter_words = std::max(scan_scratch_words(n_slots), (uint64_t)1);
    if (!s->f_slots.grow(n_slots * 8) || !s->f_letters.grow(n_slots) || !s->f_place.grow(n_slots * 4) || !s->f_words.grow(letter_words * 8))
        return no_memory("the slot table", n_slots * 13);
    s->base_bytes = (int64_t)(n_positions * 8 + n_slots * 13 + (scan_words + letter_words) * 8 + n_desc * sizeof(ChunkDesc));
    ST_HIP(hipMemsetAsync(s->f_slots.p, 0, n_slots * 8, s->stream));
    k_stitch_scatter<<<(unsigned)n_desc, ST_THREADS, 0, s->stream>>>(s->f_desc.as<ChunkDesc>(), d_pmin, d_pbase, s->f_base.as<uint32_t>(),
                                                                      s->f_slots.as<unsigned long long>(), n_positions, n_slots, d_fault);
    ST_HIP(hipGetLastError());
    const unsigned slot_blocks = (unsigned)((n_slots + ST_THREADS - 1) / ST_THREADS);
    if (slot_blocks) {
        k_stitch_check<<<slot_blocks, ST_THREADS, 0, s->stream>>>(s->f_slots.as<unsigned long long>(), n_slots, s->f_letters.as<uint8_t>(), d_bad);
        ST_HIP(hipGetLastError());
    }
    const uint64_t* d_letters_total = scan_exclusive<LoadLetter, uint32_t>(s->stream, LoadLetter{s->f_letters.as<uint8_t>()}, n_slots,
                                                                           s->f_place.as<uint32_t>(), s->f_words.as<uint64_t>());
    ST_HIP(hipGetLastError());
    uint64_t n_letters = 0;
    uint32_t flags[2] = {0, 0};
    ST_HIP(hipMemcpyAsync(&n_letters, d_letters_total, 8, hipMemcpyDeviceToHost, s->stream));
    ST_HIP(hipMemcpyAsync(flags, d_fault, 8, hipMemcpyDeviceToHost, s->stream));
    ST_HIP(hipStreamSynchronize(s->stream));
    if (flags[0]) return pa::set_error(PA_ERR_HIP, "stitcher finish: a row fell outside its piece's tables (flags " + std::to_string(flags[0]) + ")");
    if (flags[1]) {                                     // label_decoder[...] raises KeyError in the reference
        *bad_label = (int32_t)flags[1];
        return PA_OK;
    }
    // 6. the letters, piece after piece
    if (!s->f_out.grow(n_letters + 1)) return no_memory("the sequence", n_letters);
    if (qualities) {
        if (!s->f_qual.grow(n_letters + 1)) return no_memory("the qualities", n_letters);
        s->base_bytes += (int64_t)n_letters;
    }
    if (slot_blocks) {
        launch_qual(k_stitch_emit<true>, k_stitch_emit<false>, slot_blocks, s->stream, qualities ? s->f_qual.as<uint8_t>() : nullptr,
                    s->f_letters.as<uint8_t>(), s->f_place.as<uint32_t>(), s->f_slots.as<unsigned long long>(), n_slots, n_letters,
                    s->f_out.as<uint8_t>());
        ST_HIP(hipGetLastError());
    }
    k_stitch_bounds<<<(unsigned)((np + 63) / 64), 64, 0, s->stream>>>(d_pbase, n_pieces, s->f_base.as<uint32_t>(), s->f_place.as<uint32_t>(),
                                                                     n_positions, n_slots, n_letters, d_start);
    ST_HIP(hipGetLastError());
    std::vector<uint64_t> start(np + 1);
    ST_HIP(hipMemcpyAsync(start.data(), d_start, np * 8, hipMemcpyDeviceToHost, s->stream));
    ST_HIP(hipStreamSynchronize(s->stream));
    start[np] = n_letters;
    for (size_t p = 0; p < np; ++p) {
        if (piece_rows[p] == 0) continue;               // a piece without kept rows is skipped: (-1, -1, '')
        const int64_t length = (int64_t)(start[p + 1] - start[p]);
        piece_length[p] = length;
        s->pieces.push_back(PieceOut{piece_first[p], piece_last[p], (int64_t)start[p], length, (int)p});
    }
    std::stable_sort(s->pieces.begin(), s->pieces.end(), [](const PieceOut& a, const PieceOut& b) {
        return a.first != b.first ? a.first < b.first : a.last < b.last;
    });
    s->sequence_length = (int64_t)n_letters;
    s->have_qualities = qualities;
    s->have_sequence = true;
    *sequence_length = (int64_t)n_letters;
    return PA_OK;
}

int pa_stitcher_take(pa_stitcher* s, char* dst, int64_t capacity) {
    if (!s || capacity < 0 || (capacity > 0 && !dst)) return pa::set_error(PA_ERR_INVALID, "stitcher take: null or negative argument");
    std::lock_guard<std::mutex> guard(s->lock);
    return take_letters(s, s->f_fill, s->f_out, dst, capacity, "stitcher take");
}

int pa_stitcher_take_qualities(pa_stitcher* s, char* dst, int64_t capacity) {
    if (!s || capacity < 0 || (capacity > 0 && !dst)) return pa::set_error(PA_ERR_INVALID, "stitcher take qualities: null or negative argument");
    std::lock_guard<std::mutex> guard(s->lock);
    if (const int rc = needs_finish(s, "stitcher take qualities", s->have_qualities || !s->contig_qualities)) return rc;
    if (!s->have_qualities)
        return pa::set_error(PA_ERR_INVALID, "stitcher take qualities: the last finish produced none: a chunk of its contig was added "
                                             "without qualities (pa_stitcher_add_qual on every chunk asks for them), or it failed early");
    return take_letters(s, s->f_fillq, s->f_qual, dst, capacity, "stitcher take qualities");
}

// pa_stitcher_edits under the handle's lock (pa_stitcher_variants makes the records it lacks through it)
static int edits_locked(pa_stitcher* s, const char* draft, int64_t draft_length, int64_t* n_edits, int64_t* counts) {
    *n_edits = 0;
    for (int k = 0; k < 6; ++k) counts[k] = 0;
    const bool held = !draft && (s->live(FILL) || s->live(WITHHELD)) && s->draft_held == draft_length;      // the draft a fill or a gate uploaded
    if (draft_length > 0 && !draft && !held)
        return pa::set_error(PA_ERR_INVALID, "stitcher edits: null draft (only after a pa_stitcher_fill or pa_stitcher_gate of a draft of this length)");
    if (const int rc = needs_finish(s, "stitcher edits", s->have_sequence)) return rc;
    if (s->last_pieces > 0xFFFF)
        return pa::set_error(PA_ERR_INVALID, "stitcher edits: the last finish had " + std::to_string(s->last_pieces) +
                                                 " pieces, a record names 65535");
    int64_t lo = -1, hi = -1;
    for (const PieceOut& piece : s->pieces) {
        lo = lo < 0 ? piece.first : std::min(lo, piece.first);
        hi = std::max(hi, piece.last);
    }
    if (draft_length <= hi)
        return pa::set_error(PA_ERR_INVALID, "stitcher edits: the draft has " + std::to_string(draft_length) +
                                                 " letters, a piece ends at position " + std::to_string(hi));
    s->begin(CALL_EDITS);
    const size_t np = (size_t)s->last_pieces;
    if (s->pieces.empty() || s->last_slots == 0) {      // nothing was merged: no record
        s->make(EDITS, 0, 0);
        return PA_OK;
    }
    ST_HIP(hipSetDevice(s->device));
    // per piece (table order): its place in take() order and what turns a table letter offset into a take() offset; then the
    // device's answers: where a piece's records begin, the records per kind
    std::vector<int64_t> shift(np, 0);
    std::vector<uint16_t> take_index(np, 0);
    int64_t at = 0;
    for (size_t k = 0; k < s->pieces.size(); ++k) {
        const PieceOut& piece = s->pieces[k];
        shift[(size_t)piece.piece] = at - piece.offset;
        take_index[(size_t)piece.piece] = (uint16_t)k;
        at += piece.length;
    }
    const size_t span = (size_t)(hi - lo + 1);
    if (!s->e_piece.grow(RecordWords::bytes(np)) || !s->e_draft.grow(span)) return no_memory("the draft", span);
    const RecordWords w{s->e_piece.as<uint8_t>(), np};
    ST_HIP(hipMemcpyAsync(w.letter_shift(), shift.data(), np * 8, hipMemcpyHostToDevice, s->stream));
    ST_HIP(hipMemcpyAsync(w.take_index(), take_index.data(), np * 2, hipMemcpyHostToDevice, s->stream));
    ST_HIP(hipMemsetAsync(w.start(), 0, w.answer_bytes(), s->stream));
    if (!held) {
        ST_HIP(hipMemcpyAsync(s->e_draft.p, draft + lo, span, hipMemcpyHostToDevice, s->stream));
        s->draft_held = -1;                             // (behind the fill's kernels on the stream; its whole draft is gone)
    }
    EditTables t = tables_of(s, w);
    t.draft = s->e_draft.as<uint8_t>() + (held ? lo : 0);
    t.draft_lo = (uint32_t)lo;
    t.draft_span = (uint32_t)span;
    if (s->live(FILL)) {
        t.holes = s->f_holes.as<uint32_t>();
        t.lead = (uint32_t)s->fill_lead;
    }
    // count per block (f_words is the letter scan's scratch: sized for n_slots elements, free since the finish), scan the sums;
    // the one wait: the record buffer's size
    uint64_t* sums = s->f_words.as<uint64_t>();
    uint64_t total = 0, kinds[6] = {0, 0, 0, 0, 0, 0};
    if (const int rc = count_records(s, t, EditRule(), sums, w.kinds(), [] { return PA_OK; }, &total, kinds)) return rc;
    if (total > 0) {
        if (!s->e_records.grow(total * sizeof(pa_stitch_edit))) return no_memory("the edit records", total * sizeof(pa_stitch_edit));
        // the write is left in flight: take_edits, a later finish and destroy are ordered behind it on the handle's stream
        k_record_write<EditRule><<<(unsigned)scan_blocks(t.n_slots), ST_THREADS, 0, s->stream>>>(t, EditRule(), sums, total,
                                                                                                 s->e_records.as<pa_stitch_edit>(), w.start());
        ST_HIP(hipGetLastError());
    }
    s->make(EDITS, (int64_t)total, (int64_t)(total * sizeof(pa_stitch_edit)));
    *n_edits = (int64_t)total;
    for (int k = 0; k < 6; ++k) counts[k] = (int64_t)kinds[k];
    return PA_OK;
}

int pa_stitcher_edits(pa_stitcher* s, const char* draft, int64_t draft_length, int64_t* n_edits, int64_t* counts) {
    if (!s || !n_edits || !counts || draft_length < 0) return pa::set_error(PA_ERR_INVALID, "stitcher edits: null or negative argument");
    std::lock_guard<std::mutex> guard(s->lock);
    return edits_locked(s, draft, draft_length, n_edits, counts);
}

int pa_stitcher_fill(pa_stitcher* s, const char* draft, int64_t draft_length, int64_t* filled_length, int64_t* counts) {
    if (!s || !filled_length || !counts || draft_length < 0) return pa::set_error(PA_ERR_INVALID, "stitcher fill: null or negative argument");
    std::lock_guard<std::mutex> guard(s->lock);
    *filled_length = 0;
    counts[0] = counts[1] = 0;
    const bool held = !draft && s->live(WITHHELD) && s->draft_held == draft_length;      // the draft the gate uploaded
    if (draft_length > 0 && !draft && !held)
        return pa::set_error(PA_ERR_INVALID, "stitcher fill: null draft (only after a pa_stitcher_gate of a draft of this length)");
    if (const int rc = needs_finish(s, "stitcher fill", s->have_sequence)) return rc;
    if (s->last_pieces > 1)
        return pa::set_error(PA_ERR_INVALID, "stitcher fill: the last finish had " + std::to_string(s->last_pieces) +
                                                 " pieces, a filled consensus is one piece");
    const bool rows = !s->pieces.empty();
    const int64_t first = rows ? s->pieces[0].first : draft_length, last = rows ? s->pieces[0].last : -1;
    if (draft_length <= last)
        return pa::set_error(PA_ERR_INVALID, "stitcher fill: the draft has " + std::to_string(draft_length) +
                                                 " letters, the piece ends at position " + std::to_string(last));
    if (draft_length > ST_MAX_POSITION)
        return pa::set_error(PA_ERR_UNSUPPORTED, "stitcher fill: the draft has " + std::to_string(draft_length) + " letters, an offset counts 2^32 - 1");
    s->begin(CALL_FILL);                                // (asked again: counted once)
    if (!held) s->draft_held = -1;
    ST_HIP(hipSetDevice(s->device));
    const uint64_t n_positions = rows ? (uint64_t)s->last_positions : 0, n_slots = (uint64_t)s->last_slots;
    const uint64_t n_letters = (uint64_t)s->sequence_length;
    if (!s->e_draft.grow((size_t)draft_length + 1) || !s->f_holes.grow(n_positions * 4 + 4)) return no_memory("the draft", (uint64_t)draft_length);
    if (draft_length > 0 && !held) ST_HIP(hipMemcpyAsync(s->e_draft.p, draft, (size_t)draft_length, hipMemcpyHostToDevice, s->stream));
    uint64_t word = 0;                                  // runs that begin inside the piece << 32 | positions without a slot
    if (n_positions) {                                  // (f_scan is the width scan's scratch: sized for n_positions, free since)
        const uint64_t* d_total = scan_exclusive<LoadHole, uint32_t>(s->stream, LoadHole{s->f_width.as<uint32_t>()}, n_positions,
                                                                     s->f_holes.as<uint32_t>(), s->f_scan.as<uint64_t>());
        ST_HIP(hipGetLastError());
        ST_HIP(hipMemcpyAsync(&word, d_total, 8, hipMemcpyDeviceToHost, s->stream));
    }
    ST_HIP(hipStreamSynchronize(s->stream));            // the one wait: the filled buffer's size
    const uint64_t holes = word & 0xFFFFFFFFull, runs = word >> 32;
    const uint64_t lead = (uint64_t)first, trail = rows ? (uint64_t)(draft_length - last - 1) : 0;
    const uint64_t total = lead + n_letters + holes + trail;
    if (total > 0xFFFFFFFFull)
        return pa::set_error(PA_ERR_UNSUPPORTED, "stitcher fill: the filled consensus has " + std::to_string(total) + " letters, an offset counts 2^32 - 1");
    const bool qualities = s->have_qualities;
    if (!s->f_fill.grow(total + 1) || (qualities && !s->f_fillq.grow(total + 1))) return no_memory("the filled sequence", total);
    uint8_t* out = s->f_fill.as<uint8_t>();
    uint8_t* qual = qualities ? s->f_fillq.as<uint8_t>() : nullptr;
    const uint8_t* d_draft = s->e_draft.as<uint8_t>();
    // the two ends are copies; everything below is left in flight: take, edits, a later finish and destroy are ordered behind it
    if (lead) ST_HIP(hipMemcpyAsync(out, d_draft, lead, hipMemcpyDeviceToDevice, s->stream));
    if (trail) ST_HIP(hipMemcpyAsync(out + (total - trail), d_draft + last + 1, trail, hipMemcpyDeviceToDevice, s->stream));
    if (qual && lead) ST_HIP(hipMemsetAsync(qual, '!', lead, s->stream));
    if (qual && trail) ST_HIP(hipMemsetAsync(qual + (total - trail), '!', trail, s->stream));
    if (n_positions) {
        const unsigned blocks = (unsigned)((n_positions + ST_THREADS - 1) / ST_THREADS);
        launch_qual(k_stitch_fill<true>, k_stitch_fill<false>, blocks, s->stream, qual, s->f_width.as<uint32_t>(), s->f_base.as<uint32_t>(),
                    s->f_holes.as<uint32_t>(), s->f_letters.as<uint8_t>(), s->f_place.as<uint32_t>(), s->f_slots.as<unsigned long long>(),
                    d_draft + first, n_positions, n_slots, n_letters, lead, total, out);
        ST_HIP(hipGetLastError());
    }
    s->make(FILL, (int64_t)total, (int64_t)(n_positions * 4 + total * (qualities ? 2 : 1)));
    s->fill_lead = (int64_t)lead;
    s->draft_held = draft_length;
    s->fill_draft_length = draft_length;
    *filled_length = (int64_t)total;
    counts[0] = (int64_t)(runs + (lead > 0) + (trail > 0));
    counts[1] = (int64_t)(lead + holes + trail);
    return PA_OK;
}

int pa_stitcher_take_edits(pa_stitcher* s, pa_stitch_edit* dst, int64_t capacity) {
    if (!s || capacity < 0 || (capacity > 0 && !dst)) return pa::set_error(PA_ERR_INVALID, "stitcher take edits: null or negative argument");
    std::lock_guard<std::mutex> guard(s->lock);
    const int64_t n_edits = s->product[EDITS].count;
    if (!s->live(EDITS)) return pa::set_error(PA_ERR_INVALID, "stitcher take edits: pa_stitcher_edits has not run since the last finish");
    if (capacity < n_edits)
        return pa::set_error(PA_ERR_INVALID, "stitcher take edits: there are " + std::to_string(n_edits) + " records, room for " +
                                                 std::to_string(capacity));
    if (n_edits == 0) return PA_OK;
    ST_HIP(hipSetDevice(s->device));
    return take_records(s, RecordWords{s->e_piece.as<uint8_t>(), (size_t)s->last_pieces}.start(), s->e_records.as<pa_stitch_edit>(), n_edits,
                        dst, "stitcher take edits");
}

int pa_stitcher_gate(pa_stitcher* s, const char* draft, int64_t draft_length, int32_t min_phred, int64_t* piece_length,
                     int64_t* sequence_length, int64_t* counts) {
    if (!s || !sequence_length || !counts || draft_length < 0 || (draft_length > 0 && !draft))
        return pa::set_error(PA_ERR_INVALID, "stitcher gate: null or negative argument");
    std::lock_guard<std::mutex> guard(s->lock);
    if (const int rc = needs_finish(s, "stitcher gate", s->have_sequence)) return rc;
    if (!s->contig_qualities)
        return pa::set_error(PA_ERR_INVALID, "stitcher gate: a chunk of the contig was added without qualities (pa_stitcher_add_qual on "
                                             "every chunk gives the gate its phred)");
    if (min_phred < 1 || min_phred > 255)
        return pa::set_error(PA_ERR_INVALID, "stitcher gate: min_phred " + std::to_string(min_phred) + " is outside 1..255");
    if (s->live(WITHHELD) || s->live(FILL))
        return pa::set_error(PA_ERR_INVALID, std::string("stitcher gate: a ") + (s->live(WITHHELD) ? "gate" : "fill") +
                                                 " already ran since the finish (the gate comes first, once)");
    if (s->last_pieces > 0xFFFF)
        return pa::set_error(PA_ERR_INVALID, "stitcher gate: the last finish had " + std::to_string(s->last_pieces) +
                                                 " pieces, a record names 65535");
    if (s->last_pieces > 0 && !piece_length) return pa::set_error(PA_ERR_INVALID, "stitcher gate: null piece_length");
    int64_t hi = -1;
    for (const PieceOut& piece : s->pieces) hi = std::max(hi, piece.last);
    if (draft_length <= hi)
        return pa::set_error(PA_ERR_INVALID, "stitcher gate: the draft has " + std::to_string(draft_length) +
                                                 " letters, a piece ends at position " + std::to_string(hi));
    if (draft_length > ST_MAX_POSITION)
        return pa::set_error(PA_ERR_UNSUPPORTED, "stitcher gate: the draft has " + std::to_string(draft_length) + " letters, an offset counts 2^32 - 1");
    const size_t np = (size_t)s->last_pieces;
    const uint64_t n_slots = (uint64_t)s->last_slots, n_positions = (uint64_t)s->last_positions;
    ST_HIP(hipSetDevice(s->device));
    // (f_scan is the width scan's scratch, free since the finish: here it takes the block sums, sized for the slots)
    if (!s->e_draft.grow((size_t)draft_length + 1) || !s->g_piece.grow(RecordWords::bytes(np)) ||
        !s->f_scan.grow(scan_scratch_words(n_slots) * 8))
        return no_memory("the draft", (uint64_t)draft_length);
    s->begin(CALL_GATE);                                // records of the ungated consensus are gone
    s->draft_held = -1;
    for (int k = 0; k < 4; ++k) counts[k] = 0;
    if (draft_length > 0) ST_HIP(hipMemcpyAsync(s->e_draft.p, draft, (size_t)draft_length, hipMemcpyHostToDevice, s->stream));
    if (s->pieces.empty() || n_slots == 0) {            // nothing was merged: nothing to withhold
        ST_HIP(hipStreamSynchronize(s->stream));
        s->draft_held = draft_length;
        s->make(WITHHELD, 0, 0);
        for (size_t p = 0; p < np; ++p) piece_length[p] = 0;
        *sequence_length = s->sequence_length;
        return PA_OK;
    }
    const RecordWords w{s->g_piece.as<uint8_t>(), np};
    const PieceWords pw{s->f_piece.as<uint8_t>(), np};
    // the pieces' take() order is the finish's: (first, last) do not move
    std::vector<uint16_t> take_index(np, 0), order(s->pieces.size(), 0);
    for (size_t k = 0; k < s->pieces.size(); ++k) {
        take_index[(size_t)s->pieces[k].piece] = (uint16_t)k;
        order[k] = (uint16_t)s->pieces[k].piece;
    }
    ST_HIP(hipMemcpyAsync(w.take_index(), take_index.data(), np * 2, hipMemcpyHostToDevice, s->stream));
    ST_HIP(hipMemcpyAsync(w.order(), order.data(), order.size() * 2, hipMemcpyHostToDevice, s->stream));
    ST_HIP(hipMemsetAsync(w.letter_shift(), 0, w.device_bytes(), s->stream));      // (k_gate_shift writes the shifts)
    EditTables t = tables_of(s, w);
    t.draft = s->e_draft.as<uint8_t>();
    t.draft_span = (uint32_t)draft_length;
    const GateRule rule{(uint32_t)min_phred, s->f_letters.as<uint8_t>(), s->f_slots.as<unsigned long long>()};
    // 1. decide every slot, rewrite its letter, count; 2. the letters' places again, the pieces' starts; 3. scan of the counts;
    // the one wait: the sizes of the sequence and of the record buffer
    uint64_t* sums = s->f_scan.as<uint64_t>();
    uint64_t n_letters = 0, total = 0, kinds[6] = {0, 0, 0, 0, 0, 0};
    std::vector<uint64_t> start(np + 1);
    const auto places_again = [&]() -> int {
        const uint64_t* d_letters_total = scan_exclusive<LoadLetter, uint32_t>(s->stream, LoadLetter{s->f_letters.as<uint8_t>()}, n_slots,
                                                                               s->f_place.as<uint32_t>(), s->f_words.as<uint64_t>());
        ST_HIP(hipGetLastError());
        k_stitch_bounds<<<(unsigned)((np + 63) / 64), 64, 0, s->stream>>>(pw.pbase(), (int)np, s->f_base.as<uint32_t>(), s->f_place.as<uint32_t>(),
                                                                         n_positions, n_slots, ST_AT_END, pw.letter_start());      // (the end: not known yet)
        ST_HIP(hipGetLastError());
        k_gate_shift<<<1, 64, 0, s->stream>>>(w.order(), (uint32_t)order.size(), pw.letter_start(), (uint32_t)np, d_letters_total, w.letter_shift());
        ST_HIP(hipGetLastError());
        ST_HIP(hipMemcpyAsync(&n_letters, d_letters_total, 8, hipMemcpyDeviceToHost, s->stream));
        ST_HIP(hipMemcpyAsync(start.data(), pw.letter_start(), np * 8, hipMemcpyDeviceToHost, s->stream));
        return PA_OK;
    };
    if (const int rc = count_records(s, t, rule, sums, w.kinds(), places_again, &total, kinds)) return rc;
    // from here on the tables are the gated ones whatever happens: letters[] and place[] are rewritten
    s->make(WITHHELD, 0, 0);
    s->have_sequence = false;                           // (until the winner words and the sequence agree with them again)
    if (!s->f_out.grow(n_letters + 1) || !s->f_qual.grow(n_letters + 1)) return no_memory("the sequence", n_letters);
    if (total > 0 && !s->g_records.grow(total * sizeof(pa_stitch_edit))) return no_memory("the withheld records", total * sizeof(pa_stitch_edit));
    for (size_t p = 0; p < np; ++p)
        if (start[p] == ST_AT_END) start[p] = n_letters;
    start[np] = n_letters;
    for (size_t p = 0; p < np; ++p) piece_length[p] = 0;
    for (PieceOut& piece : s->pieces) {                 // (those with kept rows; their order by (first, last) stands)
        piece.offset = (int64_t)start[(size_t)piece.piece];
        piece.length = (int64_t)(start[(size_t)piece.piece + 1] - start[(size_t)piece.piece]);
        piece_length[piece.piece] = piece.length;
    }
    // 4. the records and the winner words, 5. the letters; left in flight: every later call is ordered behind them on the stream
    if (total > 0) {                                    // (nothing withheld: every table and the sequence are as they were)
        k_record_write<GateRule><<<(unsigned)scan_blocks(n_slots), ST_THREADS, 0, s->stream>>>(t, rule, sums, total,
                                                                                               s->g_records.as<pa_stitch_edit>(), w.start());
        ST_HIP(hipGetLastError());
        launch_qual(k_stitch_emit<true>, k_stitch_emit<false>, (unsigned)((n_slots + ST_THREADS - 1) / ST_THREADS), s->stream,
                    s->f_qual.as<uint8_t>(), s->f_letters.as<uint8_t>(), s->f_place.as<uint32_t>(), s->f_slots.as<unsigned long long>(),
                    n_slots, n_letters, s->f_out.as<uint8_t>());
        ST_HIP(hipGetLastError());
    }
    s->make(WITHHELD, (int64_t)total, (int64_t)(total * sizeof(pa_stitch_edit)));
    s->base_bytes += (int64_t)n_letters - s->sequence_length;      // (the quality buffer follows the sequence's length)
    s->sequence_length = (int64_t)n_letters;
    s->draft_held = draft_length;
    s->have_sequence = true;
    *sequence_length = (int64_t)n_letters;
    counts[0] = (int64_t)total;
    for (int k = 1; k < 4; ++k) counts[k] = (int64_t)kinds[k];
    return PA_OK;
}

int pa_stitcher_take_withheld(pa_stitcher* s, pa_stitch_edit* dst, int64_t capacity) {
    if (!s || capacity < 0 || (capacity > 0 && !dst)) return pa::set_error(PA_ERR_INVALID, "stitcher take withheld: null or negative argument");
    std::lock_guard<std::mutex> guard(s->lock);
    const int64_t n_withheld = s->product[WITHHELD].count;
    if (!s->live(WITHHELD) || !s->have_sequence)
        return pa::set_error(PA_ERR_INVALID, "stitcher take withheld: pa_stitcher_gate has not run since the last finish");
    if (capacity < n_withheld)
        return pa::set_error(PA_ERR_INVALID, "stitcher take withheld: there are " + std::to_string(n_withheld) + " records, room for " +
                                                 std::to_string(capacity));
    if (n_withheld == 0) return PA_OK;
    ST_HIP(hipSetDevice(s->device));
    if (s->live(FILL) && !s->withheld_filled) {         // a fill came behind the gate: the offsets count its letters, once
        k_gate_filled_offsets<<<(unsigned)((n_withheld + 255) / 256), 256, 0, s->stream>>>(
            s->g_records.as<pa_stitch_edit>(), (uint64_t)n_withheld, s->f_holes.as<uint32_t>(), (uint64_t)s->last_positions,
            (uint32_t)s->pieces[0].first, (uint32_t)s->fill_lead);
        ST_HIP(hipGetLastError());
        s->withheld_filled = true;
    }
    return take_records(s, RecordWords{s->g_piece.as<uint8_t>(), (size_t)s->last_pieces}.start(), s->g_records.as<pa_stitch_edit>(),
                        n_withheld, dst, "stitcher take withheld");
}

int pa_stitcher_variants(pa_stitcher* s, const char* draft, int64_t draft_length, int64_t* n_variants, int64_t* counts) {
    if (!s || !n_variants || !counts || draft_length < 0) return pa::set_error(PA_ERR_INVALID, "stitcher variants: null or negative argument");
    std::lock_guard<std::mutex> guard(s->lock);
    *n_variants = 0;
    for (int k = 0; k < 5; ++k) counts[k] = 0;
    if (const int rc = needs_finish(s, "stitcher variants", s->have_sequence)) return rc;
    if (!s->live(FILL))
        return pa::set_error(PA_ERR_INVALID, "stitcher variants: pa_stitcher_fill has not run since the last finish (the records describe "
                                             "the one complete consensus of the contig)");
    if (draft_length != s->fill_draft_length)
        return pa::set_error(PA_ERR_INVALID, "stitcher variants: the draft has " + std::to_string(draft_length) + " letters, the fill's had " +
                                                 std::to_string(s->fill_draft_length));
    if (!draft && draft_length > 0 && s->draft_held != draft_length)
        return pa::set_error(PA_ERR_INVALID, "stitcher variants: null draft, and the copy the fill uploaded is gone (a pa_stitcher_edits "
                                             "with a draft of its own replaced it)");
    ST_HIP(hipSetDevice(s->device));
    s->begin(CALL_VARIANTS);                            // (asked again: counted once)
    if (draft && draft_length > 0) {
        if (!s->e_draft.grow((size_t)draft_length + 1)) return no_memory("the draft", (uint64_t)draft_length);
        ST_HIP(hipMemcpyAsync(s->e_draft.p, draft, (size_t)draft_length, hipMemcpyHostToDevice, s->stream));
        ST_HIP(hipStreamSynchronize(s->stream));        // the caller's draft is free again
        s->draft_held = draft_length;
    }
    if (!s->live(EDITS)) {                              // the one comparison there is: the records of the filled consensus
        int64_t n_edits = 0, kinds[6];
        const int rc = edits_locked(s, nullptr, draft_length, &n_edits, kinds);
        if (rc != PA_OK) return rc;
    }
    const uint64_t n = (uint64_t)s->product[EDITS].count;
    if (n == 0) {
        s->make(VARIANTS, 0, 0);
        return PA_OK;
    }
    VarTables t;
    t.records = s->e_records.as<pa_stitch_edit>();
    t.draft = s->e_draft.as<uint8_t>();
    t.cons = s->f_fill.as<uint8_t>();
    t.n_records = n;
    t.draft_length = (uint64_t)draft_length;
    t.cons_length = (uint64_t)s->product[FILL].count;
    // 1. the hunks: heads by the joining rule, scanned
    if (!s->v_before.grow(n * 4) || !s->v_scan.grow(std::max(scan_scratch_words(n), (uint64_t)1) * 8) || !s->v_words.grow(64))
        return no_memory("the hunk heads", n * 4);
    const uint64_t* d_heads = scan_exclusive<LoadHead, uint32_t>(s->stream, LoadHead{t.records}, n, s->v_before.as<uint32_t>(),
                                                                 s->v_scan.as<uint64_t>());
    ST_HIP(hipGetLastError());
    uint64_t n_hunks = 0;
    ST_HIP(hipMemcpyAsync(&n_hunks, d_heads, 8, hipMemcpyDeviceToHost, s->stream));
    ST_HIP(hipStreamSynchronize(s->stream));            // the first wait: the size of the hunk tables
    int64_t bytes = (int64_t)(n * 4);
    if (n_hunks == 0) {                                  // GAP records alone
        s->make(VARIANTS, 0, bytes);
        return PA_OK;
    }
    if (n_hunks > 0xFFFFFFFEull) return pa::set_error(PA_ERR_UNSUPPORTED, "stitcher variants: more than 2^32 - 2 hunks");
    if (!s->v_hunks.grow(n_hunks * sizeof(HunkWork)) || !s->v_tmp.grow(n_hunks * sizeof(pa_stitch_variant)) || !s->v_emit.grow(n_hunks) ||
        !s->v_place.grow(n_hunks * 4) || !s->v_scan.grow(std::max(scan_scratch_words(std::max(n, n_hunks)), (uint64_t)1) * 8))
        return no_memory("the hunk tables", n_hunks * (sizeof(HunkWork) + sizeof(pa_stitch_variant) + 5));
    bytes += (int64_t)(n_hunks * (sizeof(HunkWork) + sizeof(pa_stitch_variant) + 5));
    HunkWork* hunks = s->v_hunks.as<HunkWork>();
    unsigned long long* d_counts = s->v_words.as<unsigned long long>();      // [5] counts, then F
    uint32_t* d_first_unlinked = (uint32_t*)(d_counts + 5);
    const uint32_t all_linked = (uint32_t)n_hunks;
    ST_HIP(hipMemsetAsync(hunks, 0xFF, n_hunks * sizeof(HunkWork), s->stream));
    ST_HIP(hipMemsetAsync(d_counts, 0, 5 * 8, s->stream));
    ST_HIP(hipMemcpyAsync(d_first_unlinked, &all_linked, 4, hipMemcpyHostToDevice, s->stream));
    const unsigned record_blocks = (unsigned)((n + ST_THREADS - 1) / ST_THREADS), hunk_blocks = (unsigned)((n_hunks + ST_THREADS - 1) / ST_THREADS);
    const unsigned wave_blocks = (unsigned)((n_hunks + ST_THREADS / 64 - 1) / (ST_THREADS / 64));
    k_var_ranges<<<record_blocks, ST_THREADS, 0, s->stream>>>(t.records, n, s->v_before.as<uint32_t>(), hunks, n_hunks);
    ST_HIP(hipGetLastError());
    // 2. trim, the contig's start, left-alignment
    k_var_trim<<<hunk_blocks, ST_THREADS, 0, s->stream>>>(t, hunks, n_hunks);
    ST_HIP(hipGetLastError());
    k_var_link<<<hunk_blocks, ST_THREADS, 0, s->stream>>>(hunks, n_hunks, d_first_unlinked);
    ST_HIP(hipGetLastError());
    k_var_align<<<wave_blocks, ST_THREADS, 0, s->stream>>>(t, hunks, n_hunks, d_first_unlinked, s->contig_qualities ? 1u : 0u,
                                                           s->v_tmp.as<pa_stitch_variant>(), s->v_emit.as<uint8_t>(), d_counts);
    ST_HIP(hipGetLastError());
    // 3. compaction in hunk order
    const uint64_t* d_kept = scan_exclusive<LoadLetter, uint32_t>(s->stream, LoadLetter{s->v_emit.as<uint8_t>()}, n_hunks,
                                                                 s->v_place.as<uint32_t>(), s->v_scan.as<uint64_t>());
    ST_HIP(hipGetLastError());
    uint64_t kept = 0, host_counts[5] = {0, 0, 0, 0, 0};
    ST_HIP(hipMemcpyAsync(&kept, d_kept, 8, hipMemcpyDeviceToHost, s->stream));
    ST_HIP(hipMemcpyAsync(host_counts, d_counts, 5 * 8, hipMemcpyDeviceToHost, s->stream));
    ST_HIP(hipStreamSynchronize(s->stream));            // the second wait: the size of the record buffer
    if (kept > 0) {
        if (!s->v_out.grow(kept * sizeof(pa_stitch_variant))) return no_memory("the variant records", kept * sizeof(pa_stitch_variant));
        // left in flight: take_variants, a later finish and destroy are ordered behind it on the handle's stream
        k_var_compact<<<hunk_blocks, ST_THREADS, 0, s->stream>>>(s->v_tmp.as<pa_stitch_variant>(), s->v_emit.as<uint8_t>(),
                                                                 s->v_place.as<uint32_t>(), n_hunks, kept, s->v_out.as<pa_stitch_variant>());
        ST_HIP(hipGetLastError());
    }
    bytes += (int64_t)(kept * sizeof(pa_stitch_variant));
    s->make(VARIANTS, (int64_t)kept, bytes);
    *n_variants = (int64_t)kept;
    counts[0] = (int64_t)kept;
    for (int k = 1; k < 5; ++k) counts[k] = (int64_t)host_counts[k];
    return PA_OK;
}

int pa_stitcher_take_variants(pa_stitcher* s, pa_stitch_variant* dst, int64_t capacity) {
    if (!s || capacity < 0 || (capacity > 0 && !dst)) return pa::set_error(PA_ERR_INVALID, "stitcher take variants: null or negative argument");
    std::lock_guard<std::mutex> guard(s->lock);
    const int64_t n_variants = s->product[VARIANTS].count;
    if (!s->live(VARIANTS)) return pa::set_error(PA_ERR_INVALID, "stitcher take variants: pa_stitcher_variants has not run since the last finish");
    if (capacity < n_variants)
        return pa::set_error(PA_ERR_INVALID, "stitcher take variants: there are " + std::to_string(n_variants) + " records, room for " +
                                                 std::to_string(capacity));
    if (n_variants == 0) return PA_OK;
    ST_HIP(hipSetDevice(s->device));
    ST_HIP(hipMemcpyAsync(dst, s->v_out.p, (size_t)n_variants * sizeof(pa_stitch_variant), hipMemcpyDeviceToHost, s->stream));
    ST_HIP(hipStreamSynchronize(s->stream));
    return PA_OK;
}

int pa_stitcher_stats(pa_stitcher* s, int64_t* out, int32_t n) {
    if (!s || !out || n < 0) return pa::set_error(PA_ERR_INVALID, "stitcher stats: null or negative argument");
    std::lock_guard<std::mutex> guard(s->lock);
    const int64_t v[6] = {s->rows_held, (int64_t)s->slabs.size() * ST_SLAB_ROWS * 8, s->last_slots, s->last_pieces, s->last_positions,
                          s->table_bytes()};
    for (int32_t i = 0; i < n; ++i) out[i] = i < 6 ? v[i] : 0;
    return PA_OK;
}

}  // extern "C"
