/* pepper_amd encoder C ABI -- pileup -> candidate summary images on MI355X.
 *
 * Replaces the pybind11 surface of the reference's variant encoder:
 *   PEPPER_VARIANT.RegionalSummaryGenerator(contig, region_start, region_end, reference_sequence)
 *     .generate_max_insert_summary(reads)
 *     .generate_summary(reads, min_snp_baseq, ..., candidate_window_size, feature_size, train_mode)
 *       -> list[CandidateImageSummary]
 *   pepper_variant/modules/cpp/pybind_api.h:55-62,73-101; region_summary.h:88-111,159-206;
 *   implementation region_summary.cpp:69-96 (axes), 174-191 (reference row), 337-566 (per-read
 *   walk), 568-916 (thresholds, candidate windows).
 * Reads arrive as flat arrays (the fields of type_read / CigarOp, read.h:52-64, cigar.h:30-53)
 * instead of per-read Python objects.  The whole per-read walk, the threshold/clamp pass and the
 * candidate window gather run as HIP kernels; the allele-string bookkeeping (ordered maps of
 * candidate strings) stays on the host, as in SURVEY.md section 7 step 7.
 * MANY REGIONS PER CALL (pa_encoder_generate_summary_batch) is the form that fills the chip: one
 * workgroup owns one 512-position tile of one region, a 100 kb region has ~200 of them.
 */
#ifndef PEPPER_AMD_ENCODER_H
#define PEPPER_AMD_ENCODER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int64_t region_start, region_end;   /* generator's ref_start / ref_end (inclusive)               */
    const char* reference;              /* reference_sequence covering [region_start, region_end]    */
    int64_t reference_len;
    int32_t n_reads;
    const int64_t* read_pos;            /* type_read.pos                                              */
    const uint8_t* read_reverse;        /* type_read.flags.is_reverse                                 */
    const int32_t* read_mapq;           /* type_read.mapping_quality (reads with mapq <= 0 are skipped) */
    const int64_t* seq_offset;          /* [n_reads+1] offsets into seq / qual                        */
    const char* seq;                    /* concatenated type_read.sequence                            */
    const uint8_t* qual;                /* concatenated type_read.base_qualities                      */
    const int64_t* cigar_offset;        /* [n_reads+1] offsets into cigar_op / cigar_len              */
    const int32_t* cigar_op;            /* CIGAR_OPERATIONS codes (cigar.h:17-27)                     */
    const int32_t* cigar_len;
} pa_pileup;

typedef struct {                        /* arguments of generate_summary, region_summary.h:191-206    */
    double min_snp_baseq, min_indel_baseq;
    double snp_freq_threshold, insert_freq_threshold, delete_freq_threshold;
    double min_coverage_threshold;
    double snp_candidate_freq_threshold, indel_candidate_freq_threshold, candidate_support_threshold;
    int32_t skip_indels;
    int64_t candidate_region_start, candidate_region_end;
    int32_t candidate_window_size;      /* ImageSizeOptions.CANDIDATE_WINDOW_SIZE = 32                */
    int32_t feature_size;               /* ImageSizeOptions.IMAGE_HEIGHT = 26                         */
} pa_summary_params;

typedef struct pa_encoder pa_encoder;

/* One encoder per (thread, GPU): owns a stream (or uses hip_stream) and reusable workspace. */
int pa_encoder_create(int32_t device, void* hip_stream, pa_encoder** out);
void pa_encoder_destroy(pa_encoder* e);

/* Encode one region.  On success *n_candidates = number of CandidateImageSummary the reference
 * would return (train_mode=False); results stay in the handle until the next call. */
int pa_encoder_generate_summary(pa_encoder* e, const pa_pileup* pileup, const pa_summary_params* params,
                                int64_t* n_candidates);

/* Many regions per launch: pileups[n_regions], params[n_regions] (one window size and one feature size per batch),
 * n_candidates[n_regions] (may be NULL).  Results are those of region 0, then region 1, ... in pa_encoder_get_results.
 * The buffers behind `pileups` (reference, seq) must stay valid until the call returns: candidate allele strings are
 * cut from them on the host. */
int pa_encoder_generate_summary_batch(pa_encoder* e, int32_t n_regions, const pa_pileup* pileups,
                                      const pa_summary_params* params, int64_t* n_candidates);
/* The two halves of the call above, for a caller that keeps a batch resident in HBM: stage = validate + upload,
 * run = kernels + host candidate enumeration + window gather (may be repeated; the pileup buffers must outlive the
 * last run).  bench.py times pa_encoder_run_staged. */
int pa_encoder_stage_batch(pa_encoder* e, int32_t n_regions, const pa_pileup* pileups, const pa_summary_params* params);
int pa_encoder_run_staged(pa_encoder* e, int64_t* n_candidates);
/* ------------------------------------------------------------------------------------------
 * The packed form: reads as BAM stores them, clipped and decoded ON THE DEVICE.
 * replaces, for the image generator: BAM_handler.get_reads per region (bam_handler.cpp:176-303, the walk that clips a
 * read to the region and decodes its bases) + the hand-over of the clipped reads above.  pa_bam_pack_regions
 * (include/pepper_amd_io.h) fills the arena and the tables for a run of regions; here they are uploaded with one copy each and
 * unpack_clip_kernel (one wave per (read, region)) produces what pa_encoder_stage_batch would have been given.  Results are
 * those of the host-clipped form bit for bit.  Nothing in the call waits for the device; pa_encoder_run_staged follows.
 *   arena        what pa_bam_pack_regions wrote (pa_encoder_host_arena returns a page-locked block of the handle for it:
 *                the upload is then asynchronous; any host memory works); NULL: the span pa_encoder_inflate_bgzf left on
 *                the device (data_off then need not be aligned)
 *   reads        n_reads table entries; pair_read[region_pairs[r] .. region_pairs[r + 1]) = the reads of region r
 *                (a read whose bases do not follow its operations: pa_encoder_set_seq_offsets before this call)
 *   regions      per region the generator's ref_start / ref_end (= the fetch range given to the packer) and its reference
 * The `reference` buffers must stay valid until the run returns (deleted bases of candidate alleles are cut from them).
 * An operation of 2^24 bases or more fails the run with PA_ERR_UNSUPPORTED: take the host-clipped form for that batch.
 * ------------------------------------------------------------------------------------------ */
#ifndef PA_PACKED_READ_DEFINED
#define PA_PACKED_READ_DEFINED
typedef struct {
    int64_t data_off;      /* in the arena: n_cigar uint32 (len << 4 | op), (l_seq + 1) / 2 bytes of 4-bit bases, l_seq qualities */
    int32_t pos;           /* 0-based leftmost position of the record */
    int32_t n_cigar;
    int32_t l_seq;
    int32_t flags;         /* BAM flag | mapping quality << 16 */
} pa_packed_read;
#endif
typedef struct {
    int64_t region_start, region_end;
    const char* reference;
    int64_t reference_len;
} pa_packed_region;
void* pa_encoder_host_arena(pa_encoder* e, int64_t bytes);      /* page-locked, grows, valid until the next call with more bytes */
int pa_encoder_stage_packed(pa_encoder* e, int32_t n_regions, const pa_packed_region* regions, const pa_summary_params* params,
                            const uint8_t* arena, int64_t arena_bytes, const pa_packed_read* reads, int32_t n_reads,
                            const int32_t* pair_read, const int32_t* region_pairs);
/* The arena filled ON THE DEVICE from the file's own bytes: the BGZF members of a span (pa_bam_read_span, include/
 * pepper_amd_io.h, fills `comp` -- pa_encoder_host_span returns a second page-locked block for it -- and the four tables) are
 * inflated into the encoder's device arena, one wavefront per member (csrc/inflate.hip; what htslib's bgzf_read_block does
 * beneath sam_itr_next, bam_handler.cpp:341-372), and copied to host_out (NULL: not) for the host's record walk
 * (pa_bam_pack_inflated, whose data_off are offsets into exactly these bytes).  pa_encoder_stage_packed with arena = NULL then
 * takes the bytes where they are.  A malformed member fails the call (PA_ERR_INVALID, the member and the reason in
 * pa_last_error), and so does a member whose inflated bytes do not have the CRC-32 of its trailer (include/
 * pepper_amd_io_device.h: checked when the trailer lies inside `comp`).  Timings: [10] the inflate kernel (HIP events),
 * [11] the whole call on the host clock (upload, kernel, download). */
void* pa_encoder_host_span(pa_encoder* e, int64_t bytes);
int pa_encoder_inflate_bgzf(pa_encoder* e, const uint8_t* comp, int64_t comp_bytes, int32_t n_blocks, const int64_t* comp_off,
                            const int32_t* comp_len, const int64_t* out_off, const int32_t* out_len, int64_t out_bytes,
                            uint8_t* host_out);
/* The BAM records of the span pa_encoder_inflate_bgzf left on the device, read out THERE: 40 bytes per record
 * (pa_record_header, include/pepper_amd_io.h: where its CIGAR / bases / qualities lie, position, counts, flags, the reference
 * bases its operations cover) instead of the span itself back over PCIe -- pa_encoder_inflate_bgzf with host_out = NULL, then
 * this, then pa_bam_pack_headers.  entries: record starts inside the span, ascending (pa_bam_span_entries: the first record and
 * the linear index's entry of every later 16 kb window); one lane follows the records from each entry up to the next, at
 * most cap_per_entry of them.  flags[0] != 0: nothing was copied -- 1 a lane ran out of slots, 2 a record shorter than its
 * core fields, 4 more records than headers_cap; flags[1] = 1: the span ends inside a record (what the walk of
 * pa_bam_pack_inflated treats as a cut).  The caller then takes the span to the host after all. */
int pa_encoder_walk_records(pa_encoder* e, int64_t data_bytes, const int64_t* entries, int32_t n_entries, int32_t cap_per_entry,
                            void* headers, int64_t headers_cap, int64_t* n_headers, int32_t* flags);
/* The read and pair tables of a run of regions built ON THE DEVICE from those headers: what pa_bam_pack_headers (include/
 * pepper_amd_io.h) does on the host after a download of 40 bytes per record, and the per-pair offsets pa_encoder_stage_packed
 * sums on the host, by two kernels over the header table where the walk left it (csrc/encoder.hip: pack_scan_kernel,
 * pack_fill_kernel; the per-record rules are csrc/pack_rule.h, the text pa_bam_pack_headers is compiled from).  A summary of a
 * few hundred bytes comes back; the clip kernel reads the device-built tables.
 * pa_encoder_submit_walk   pa_encoder_walk_records without its wait and without the download of the headers: the walk is
 *                     queued, nothing is returned.  pa_encoder_pack_records (headers = NULL) follows in the same submission
 *                     and waits ONCE for both; out->walk_flags are the walk's flags, out->n_headers its record count.
 * pa_encoder_walk_headers  the headers and flags of the handle's last walk after all (the caller's way back to
 *                     pa_bam_pack_headers when the pack hands a span back).
 * pa_encoder_pack_records  headers == NULL: the table the handle's last walk left on the device; otherwise n_headers host
 *                     entries (pa_record_header) are uploaded first (tests, callers with their own walk).  ref_id = the
 *                     contig's index in the BAM header, start / stop / include_supplementary / min_mapq as for
 *                     pa_bam_pack_headers, reads_cap / pairs_cap = the table sizes the host walk would be given.  Every kept
 *                     read's slice(s) are checked against the resident span here, before any kernel dereferences them (both
 *                     slices of a state-3 record; pa_encoder_set_split_slices says whether those are kept at all).
 *                     out->status == 0: region_pairs [n_regions + 1], n_done, the counts and the tables
 *                     pa_encoder_packed_tables returns equal byte for byte what pa_bam_pack_headers returns with rc 0 on the
 *                     same headers and arguments; a cut that closed at least one region is status 0 with n_done < n_regions.
 *                     out->status != 0: nothing usable, and the verdict is the host walk's (the device may report a case the
 *                     host walk would have stopped in front of).  Two such cases are known and deliberate.  The slice, CG
 *                     and cap checks (statuses 5, 3, 1) cover every kept read up to the walk's end, also the reads behind
 *                     the header that closed the last closed region of a cut span, which the host walk does not keep.  And a
 *                     state-2 header of an earlier contig gives status 2, where the host walk skips it with the rest of that
 *                     contig.  In both the host walk may return 0 for a span the device handed back; pa_encoder_pack_calls
 *                     (the driver's host_packed_calls) shows how often that happens on real spans.
 *                     Device memory: the first call allocates the handle's tables for reads_cap reads (24 + 8 + 8 bytes
 *                     each) and pairs_cap pairs (24 + 4 bytes each), sized by the caps and not by the span, and they stay
 *                     with the handle.
 * pa_encoder_stage_packed_device  pa_encoder_stage_packed of the out->n_done regions over the tables the last
 *                     pa_encoder_pack_records left (the span still resident): the same uploads and launches, without the
 *                     read, pair and offset tables.  pa_encoder_run_staged follows.
 * pa_encoder_packed_tables  the device-built tables copied out (any pointer may be NULL): n_reads reads and base offsets,
 *                     n_pairs pair_read entries.
 * pa_encoder_pack_calls  calls of this handle packed on the device / handed back with status != 0 (either may be NULL). */
typedef struct {
    int32_t status;        /* 0: tables complete.  != 0: nothing usable, the caller takes pa_bam_pack_headers:
                              1 reads_cap / pairs_cap exceeded, 2 a header in state 2 before the walk's end,
                              3 a kept header in state 1 (or state 3 with split slices off), 4 cut before the first region closed,
                              5 a kept read's slice outside the span / a size limit, 6 the walk left no table (walk_flags[0]) */
    int32_t n_done, n_reads, n_pairs, n_split;
    int32_t walk_flags[2]; /* headers == NULL: flags[0..1] of pa_encoder_walk_records */
    int32_t reserved;
    int64_t n_headers;     /* headers the pack looked at */
    int64_t slice_bytes;   /* counts[2] of pa_bam_pack_headers */
    int64_t total_bases, total_ops;      /* room the clipped pairs of the closed regions are given */
} pa_device_pack;
int pa_encoder_submit_walk(pa_encoder* e, int64_t data_bytes, const int64_t* entries, int32_t n_entries, int32_t cap_per_entry);
int pa_encoder_walk_headers(pa_encoder* e, void* headers, int64_t headers_cap, int64_t* n_headers, int32_t* flags);
int pa_encoder_pack_records(pa_encoder* e, const void* headers, int64_t n_headers, int32_t data_is_final, int32_t ref_id,
                            int32_t n_regions, const int64_t* start, const int64_t* stop, int32_t include_supplementary,
                            int32_t min_mapq, int32_t reads_cap, int32_t pairs_cap, int32_t* region_pairs, pa_device_pack* out);
int pa_encoder_stage_packed_device(pa_encoder* e, int32_t n_regions, const pa_packed_region* regions, const pa_summary_params* params);
int pa_encoder_packed_tables(pa_encoder* e, pa_packed_read* reads, int32_t* pair_read, int64_t* seq_off);
int pa_encoder_pack_calls(pa_encoder* e, int64_t* on_device, int64_t* handed_back);
/* Reads whose CIGAR travels in the CG tag, kept on the device path (both off / empty on a new handle).
 * pa_encoder_set_split_slices  on != 0: pa_encoder_walk_records looks the tag up in the record's auxiliary fields (one wavefront
 *                     per record; every byte read lies inside the record and the span) and reports state 3 as
 *                     include/pepper_amd_io.h describes instead of state 1; a malformed field gives state 2.
 * pa_encoder_set_seq_offsets  seq_off[k] for each of the n_reads packed reads of the NEXT pa_encoder_stage_packed /
 *                     pa_polish_chain_run: where read k's `bases | qualities` lie in the arena when they do not follow its
 *                     operations, -1 when they do (pa_bam_split_offsets fills it).  The table is copied, serves that one call
 *                     (which checks both slices against the arena and fails when n_reads differs from its own) and is then
 *                     forgotten, whether the call succeeded or was refused; NULL with n_reads = 0 clears it. */
int pa_encoder_set_split_slices(pa_encoder* e, int32_t on);
int pa_encoder_set_seq_offsets(pa_encoder* e, const int64_t* seq_off, int32_t n_reads);
/* Host threads of a run's candidate enumeration (one short task per region): 0 = the default (the CPUs the process may use),
 * 1 = the calling thread alone -- what image generation sets, whose workers each drive their own encoder while the other
 * CPUs inflate BGZF blocks. */
int pa_encoder_set_host_threads(pa_encoder* e, int32_t n);
/* Reads with at least one base inside each region of the last run -- the reference's len(all_reads) after get_reads (an
 * interval without any writes no summary group, AlignmentSummarizer.py:200-204); host-clipped form: the pileup's n_reads. */
int pa_encoder_region_reads(pa_encoder* e, int32_t* n_reads, int32_t n);
/* The reference's reservoir sample of deep intervals, drawn ON THE DEVICE for the packed forms (pa_encoder_run_staged after
 * pa_encoder_stage_packed, pa_polish_chain_run): an interval whose n reads with a base inside exceed
 * k = int(min(max_reads, rate * n)) keeps the k reads numpy.random.RandomState(seed) picks in read order
 * (AlignmentSummarizer.py: 192-199 variant, 314-326 polish; csrc/reservoir.h), between the clip and everything that reads the
 * pairs (reservoir_keep_kernel: one workgroup per such interval).  The region-read counts are then those AFTER sampling; an
 * interval with k == 0 keeps nothing.  Off at creation; takes effect from the handle's next run; max_reads == 0 switches it
 * off again, 1 <= max_reads <= 5000 (the slots live in LDS), rate >= 0 (the polish caller gives 1.0: k = max_reads).  The
 * kernel is not launched for a call in which no interval can need it (rate >= 1 and no interval with more than max_reads pairs).
 * pa_encoder_sampled_regions: intervals sampled and reads dropped by this handle since it was created (either may be NULL).
 * pa_encoder_pair_live: keep[p] = 1 where (read, region) pair p of the last packed batch still counts as a read of its interval
 * (a base inside and, if the interval was sampled, kept), for the first n pairs. */
int pa_encoder_set_sampling(pa_encoder* e, uint32_t seed, int32_t max_reads, double rate);
int pa_encoder_sampled_regions(pa_encoder* e, int64_t* regions, int64_t* reads_dropped);
int pa_encoder_pair_live(pa_encoder* e, uint8_t* keep, int64_t n);

/* The candidates of a run enumerated ON THE DEVICE (off on a new handle; callable between calls; holds for every variant form:
 * pa_encoder_generate_summary[_batch], pa_encoder_run_staged after pa_encoder_stage_batch or pa_encoder_stage_packed).  Off, a run
 * waits for its counts, copies sites, votes, the rare-alphabet list and the allele pool to the host, orders and enumerates them
 * there, uploads the candidate table and waits again for the windows.  On, group_votes_kernel and enumerate_sites_kernel
 * (csrc/encoder.hip; order and rule from csrc/candidates.h, the text the host enumeration is compiled from) produce the same
 * table, positions, depths, frequencies and names in device memory and the window gather follows in the same submission: one
 * wait per run, results byte for byte those of the host enumeration.  pa_encoder_get_results fetches the lists from the device
 * when asked.  A run the kernels do not take -- a site with more than 1024 indel votes, or with more than twelve distinct read
 * letters outside ACGT -- is enumerated on the host exactly as with the switch off, after the one wait.
 * pa_encoder_candidate_calls: runs of this handle (switch on) enumerated on the device / handed back to the host; either may be
 * NULL. */
int pa_encoder_set_device_candidates(pa_encoder* e, int32_t on);
int pa_encoder_candidate_calls(pa_encoder* e, int64_t* on_device, int64_t* on_host);

/* Targets of the contig the next calls' regions lie on: n disjoint, ascending, non-touching half-open intervals
 * [start[i], end[i]) in contig coordinates.  A position outside all of them carries no candidate (it fails the
 * per-position pass as if outside candidate_region_start.._end); summary matrix and windows are unchanged.
 * n == 0: no restriction (the state of a new handle).  The table is copied to the device in this call and holds for every
 * later stage / run of the handle, pa_encoder_run_staged repeated included, until set again.  A table that is not of that
 * form (start >= end, a negative start, an interval that does not begin behind the end of the one before it) is refused with
 * PA_ERR_INVALID, pa_last_error names the interval's index, and the handle keeps the table it had.  With a table set,
 * target_rows_kernel (csrc/encoder.hip) writes one verdict per matrix row in front of tile_count_kernel, which reads it in its
 * per-position pass; without one it is not launched.  The polish encoder and the polish chain ignore the table. */
int pa_encoder_set_targets(pa_encoder* e, int64_t n, const int64_t* start, const int64_t* end);

/* Two per-position tracks, depth classes and reference blocks (below), share one scheme in csrc/encoder.hip: the rows of every
 * region's candidate window classified by at most 8 ascending lower bounds (ClassBounds / class_of), the classes run-length
 * encoded per 512-row tile in a COUNT and an EMIT launch around tile_offsets_kernel (track_row, note_heads, head_rank), the
 * records sized, re-emitted on overflow and counted by submit_track / finish_track over a RunTrack of the batch, and fetched
 * with the ends derived by fetch_track.  What differs is said with each: where a run may begin, and what a record carries.
 *
 * Depth classes of the positions a run looked at (opt-in, not in the reference; pepper_amd/variant/Coverage.py is the host twin
 * and writes the BED).  The depth of a position is what tile_count_kernel holds as its coverage when the per-position pass
 * starts -- the reference's coverage_vector (region_summary.cpp:379, :454): aligned bases with quality >= min_snp_baseq and
 * insert anchors rescued by the indel quality rule, of reads with mapping quality > 0, after the reservoir sample where one
 * was drawn; deleted bases do not count -- the number `cov < min_coverage_threshold` refuses a site by.
 * pa_encoder_set_depth_bins  n ascending lower bounds, lower[0] == 0 < lower[1] < ... , 1 <= n <= 8: bin k holds the depths in
 *                     [lower[k], lower[k + 1]), the last bin is open above.  n == 0: off (the state of a new handle; every launch
 *                     and every output byte is then as without the feature).  Holds for every variant form -- pa_encoder_
 *                     generate_summary[_batch], pa_encoder_run_staged after pa_encoder_stage_batch, pa_encoder_stage_packed or
 *                     pa_encoder_stage_packed_device, repeated runs included -- until set again.  n > 8, lower[0] != 0 or a bound
 *                     not above the one before it: PA_ERR_INVALID, pa_last_error names the entry, the handle keeps what it had.
 *                     With bins set tile_count_kernel (its TILE_DEPTH instance) stores every row's depth (int32, four bytes per row beside the 104 of the
 *                     matrix: no saturation, any int32 bound is taken), and behind the run's other kernels, in the same submission
 *                     and before its one wait, depth_runs_kernel (csrc/encoder.hip; one workgroup per 512-row tile, run twice around
 *                     a scan of the tiles' counts) run-length encodes the bins of the rows of every region's candidate window
 *                     [candidate_region_start, candidate_region_end] cut to the region: one 12-byte record per run stays on the
 *                     device, 72 bytes of totals per region come back with the run's counters.
 *                     With targets set (pa_encoder_set_targets) a position outside all of them has bin -1: its runs are
 *                     reported like any other, the totals leave them out.  Candidates and images do not depend on the bins.
 *                     Room for the records is one per 16 rows and four per tile (a sixteenth of the worst case, a run per
 *                     row), or what an earlier run of the handle needed; a run with more is emitted a second time into a
 *                     buffer of the scanned total after one more wait, and counted (pa_encoder_depth_calls): the answer is exact
 *                     either way.  Debug: PEPPER_AMD_DEPTH_RUN_CAP=<records>, read by this call, replaces the first figure.
 * pa_encoder_depth_runs  *n_runs = the runs of the last run (all regions, in region and position order; valid until the
 *                     handle's next stage or run).  With any of region / start / end / bin given, capacity >= *n_runs entries
 *                     are filled -- one download of the records, the ends derived here: region index, start and end (half-open)
 *                     as contig positions, bin -- else PA_ERR_INVALID (nothing is truncated).  PA_ERR_INVALID too when the last
 *                     run had no bins set.
 * pa_encoder_depth_totals  per region r < n_regions of the last run: bases[8 r + k] positions of its window in bin k
 *                     (on-target ones when targets are set), depth_sum[r] the sum of their depths; either may be NULL.
 * pa_encoder_depth_calls  runs of this handle made with bins set / runs among them emitted twice (either may be NULL). */
int pa_encoder_set_depth_bins(pa_encoder* e, int32_t n, const int32_t* lower);
int pa_encoder_depth_runs(pa_encoder* e, int64_t capacity, int32_t* region, int64_t* start, int64_t* end, int32_t* bin, int64_t* n_runs);
int pa_encoder_depth_totals(pa_encoder* e, int32_t n_regions, int64_t* bases, int64_t* depth_sum);
int pa_encoder_depth_calls(pa_encoder* e, int64_t* runs_with_bins, int64_t* overflows);

/* Reference blocks of the positions a run looked at (opt-in, not in the reference; pepper_amd/variant/RefConfidence.py states the
 * rule and builds the table, pepper_amd/variant/Gvcf.py writes the gVCF).  Per position, from tile_count_kernel's counters
 * before the int8 clamp and the sign flip (F / R: forward / reverse slot of a symbol): cov the coverage above, ref_col = F + R
 * of the reference letter (0 where it is not one of ACGT), ins = F + R of the insert anchor, star = F + R of `*`;
 * n_ref = max(0, ref_col - ins), n_alt = max(0, cov - ref_col) + min(ins, ref_col) + star; with n = n_ref + n_alt > 100 both are
 * rescaled in 64-bit integers, n_ref' = (100 n_ref + n - 1) / n, n_alt' = 100 - n_ref'.  GQ = table[n_ref][n_alt], 0 where the
 * reference letter is not one of ACGT: a read-count model (DeepVariant's reference confidence), not the network's output.
 * pa_encoder_set_ref_confidence  table: table_side x table_side uint8, row n_ref, column n_alt (HOST pointer, copied to the
 *                     device by this call); table_side must be 101.  lower: n_bands ascending lower bounds of GQ,
 *                     lower[0] == 0 < lower[1] < ... <= 255, 1 <= n_bands <= 8: band k holds the GQs in [lower[k], lower[k + 1]),
 *                     the last band is open above.  n_bands == 0: off (the state of a new handle; every launch and every
 *                     output byte is then as without the feature; table and lower are not read).  Holds for every variant form
 *                     -- pa_encoder_generate_summary[_batch], pa_encoder_run_staged after any staging call, repeated runs
 *                     included -- until set again.  Malformed: a side other than 101, more than 8 bands, lower[0] != 0, a bound
 *                     not above the one before it or above 255, table[0][0] != 0, an entry below the one of one reference read
 *                     less or above the one of one other read less -- PA_ERR_INVALID, pa_last_error names the entry, the
 *                     handle keeps what it had.
 *                     With a table set tile_count_kernel (its third instance; it serves the depth bins too when both are set)
 *                     stores every row's depth (int32, no saturation) and GQ (one byte), and behind the run's other kernels, in
 *                     the same submission and before its one wait, ref_blocks_kernel (csrc/encoder.hip; one workgroup per
 *                     512-row tile, run twice around a scan of the tiles' counts) run-length encodes the bands of the rows of
 *                     every region's candidate window cut to the region, with the smallest depth and the smallest GQ of each
 *                     run: one 20-byte record per run and tile stays on the device, their count comes back with the run's
 *                     counters.  A run that crosses a tile border (every 512 rows of a region) is reported as one record per
 *                     tile: touching records of equal band are the caller's to merge, taking the minima (RefConfidence.py
 *                     merge_blocks).  With targets set a position outside all of them has band -1 and is reported like any
 *                     other.  Candidates and images do not depend on the table.
 *                     Room for the records is sized as for the depth runs, or by what an earlier run of the handle needed; a
 *                     run with more is emitted a second time after one more wait, exact, and counted (pa_encoder_ref_calls).
 *                     Debug: PEPPER_AMD_REF_BLOCK_CAP=<records>, read by this call, replaces the first figure.
 * pa_encoder_ref_blocks  *n_blocks = the records of the last run (all regions, in region and position order; valid until the
 *                     handle's next stage or run).  With any output array given, capacity >= *n_blocks entries are filled --
 *                     region index, start and end (half-open) as contig positions, band, smallest depth, smallest GQ -- else
 *                     PA_ERR_INVALID (nothing is truncated).  PA_ERR_INVALID too when the last run had no table set.
 * pa_encoder_ref_calls  runs of this handle made with a table set / runs among them emitted twice (either may be NULL). */
int pa_encoder_set_ref_confidence(pa_encoder* e, const uint8_t* table, int32_t table_side, int32_t n_bands, const int32_t* lower);
int pa_encoder_ref_blocks(pa_encoder* e, int64_t capacity, int32_t* region, int64_t* start, int64_t* end, int32_t* band, int32_t* min_dp,
                          int32_t* min_gq, int64_t* n_blocks);
int pa_encoder_ref_calls(pa_encoder* e, int64_t* runs, int64_t* overflows);

/* Times of the last run in milliseconds, HIP events on the encoder's stream: [0] record kernels (segment_reads x 2 +
 * tile_offsets), [1] tile_count_kernel, [2] compact_votes_kernel + pack_results_kernel, [3] gather_windows_kernel; host clock:
 * [4] candidate enumeration, [5] the whole run, [6], [7] parts of [4]; packed form: [8] upload of arena + tables,
 * [9] unpack_clip_kernel; [12] the device enumeration (group_votes_kernel, enumerate_sites_kernel and the scans between them;
 * [4], [6], [7] are 0 for a run it served, [12] is 0 for every other run); [13] the depth-class kernels (depth_runs_kernel twice and the
 * scan between them, HIP events; 0 for a run without depth bins); [14] the reference-block kernels (ref_blocks_kernel twice and
 * the scan between them, HIP events; 0 for a run without a reference-confidence table).  Sizes of the staged batch: [0] read bases, [1] matrix rows,
 * [2] reads, [3] CIGAR operations, [4] tiles, [5] regions. */
int pa_encoder_last_timing(pa_encoder* e, double* ms, int32_t n);
int pa_encoder_batch_stats(pa_encoder* e, int64_t* out, int32_t n);

/* Copy results of the last call (HOST pointers, any may be NULL):
 *   positions int64 [n], depths int32 [n], candidate_frequency int32 [n]  (CandidateImageSummary
 *   .position / .depth / .candidate_frequency[0]); images_i32 [n, window+1, feature] = image_matrix;
 *   images_i8 = the same values wrapped to int8 exactly as DataStore.py:68 stores them;
 *   candidates: n NUL-terminated allele strings (.candidates[0]); *candidates_needed = bytes. */
int pa_encoder_get_results(pa_encoder* e, int64_t* positions, int32_t* depths, int32_t* candidate_frequency,
                           int32_t* images_i32, int8_t* images_i8, char* candidates, int64_t candidates_cap,
                           int64_t* candidates_needed);

/* Device pointer to the int8 images of the last call ([n, window+1, feature], valid until the
 * next call) so inference can consume them without a host round trip. */
const int8_t* pa_encoder_device_images(pa_encoder* e);

/* ------------------------------------------------------------------------------------------
 * Polish summary encoder
 * replaces: PEPPER.SummaryGenerator(ref_seq, chr, start, end).generate_summary(reads, start, end)
 *   -> .image (uint8 rows of 10 features), .genomic_pos ((position, insert index) per row)
 *   pepper/modules/headers/pybind_api.h:18-25; pepper/modules/src/pileup_summary/summary_generator.cpp:
 *   16-32 (feature index), 47-121 (per-read walk), 274-306 (pixels), 370-393 (row order).
 * pileup->region_start/end = the constructor's ref_start/ref_end; start_pos/end_pos = the
 * arguments of generate_summary (identical in the reference's caller, AlignmentSummarizer.py:340-347).
 * ------------------------------------------------------------------------------------------ */
int pa_polish_encoder_generate_summary(pa_encoder* e, const pa_pileup* pileup, int64_t start_pos,
                                       int64_t end_pos, int64_t* n_rows);
/* Many regions per launch: pileups[n_regions], start_pos[n_regions], end_pos[n_regions] -> n_rows[n_regions] (may be NULL);
 * the results are the rows of region 0, then region 1, ...  The whole per-read walk runs on the device. */
int pa_polish_encoder_generate_summary_batch(pa_encoder* e, int32_t n_regions, const pa_pileup* pileups,
                                             const int64_t* start_pos, const int64_t* end_pos, int64_t* n_rows);
/* The two halves of the call above (stage = validate + upload, run = the kernels; may be repeated: what bench.py times with the
 * pileups resident in HBM), and the sizes of the staged batch / last run: [0] read bases, [1] output rows, [2] reads, [3] CIGAR
 * operations, [4] tiles, [5] regions, [6] the launch sets the last run took: 1 where the first sizes of the record and
 * insert-slot buffers held, 2 or 3 where the run was repeated with room (0 before any run). */
int pa_polish_encoder_stage_batch(pa_encoder* e, int32_t n_regions, const pa_pileup* pileups, const int64_t* start_pos,
                                  const int64_t* end_pos);
int pa_polish_encoder_run_staged(pa_encoder* e, int64_t* n_rows);
int pa_polish_encoder_batch_stats(pa_encoder* e, int64_t* out, int32_t n);
/* HOST pointers: image uint8 [n_rows, 10], positions int64 [n_rows, 2] (of all regions of the last call); either may be NULL. */
int pa_polish_encoder_get_results(pa_encoder* e, uint8_t* image, int64_t* positions);
/* HIP-event times of the last call in ms: [0] record / scan kernels, [1] polish_tile_kernel, [2] polish_insert_rows_kernel. */
int pa_polish_encoder_last_timing(pa_encoder* e, double* ms, int32_t n);

/* ------------------------------------------------------------------------------------------
 * The polish image chain: BAM records -> image chunks of N regions without a host hop in between.
 * replaces, per region: AlignmentSummarizer.create_summary's inference branch --
 *   bam_handler.get_reads(chr, start, end, False, 0, 0)            pepper/modules/python/AlignmentSummarizer.py:296-303
 *   reads_to_reference_realignment (ReadAligner over every read)   :159-177, 328-332; simple_aligner.cpp:66-106
 *   SummaryGenerator(...).generate_summary(reads, start, end)      :334-347; summary_generator.cpp:47-121, 274-306, 370-393
 *   chunk_images(summary, 1000, 50)                                :18-56
 * The reads arrive in the packed form of pa_encoder_stage_packed (or are the span pa_encoder_inflate_bgzf left on the device:
 * arena = NULL); unpack_clip_kernel clips and decodes them per (read, region), the re-aligner (include/pepper_amd_realign.h)
 * takes them from there and leaves positions and CIGARs on the device, the summary encoder reads those, and the rows are cut
 * into chunks of chunk_size rows (the next one starting chunk_overlap rows before the end of the previous one, the last one
 * padded with zero rows and (-1, -1) positions) by a kernel.  One download: the chunks.
 *   regions[r]   region_start / region_end = the region (reads fetched from it, summary over it); reference / reference_len =
 *                the draft from region_start to region_end + ALIGNMENT_SAFE_BASES (20), shorter at the contig's end: the
 *                re-aligner's window (ignored when realign == 0)
 *   realign      realignment_flag of create_summary
 * Outputs (any may be NULL): n_rows[r] summary rows, region_reads[r] = the reference's len(all_reads), n_chunks[r] (0 for a
 * region without reads: it writes nothing), *total_chunks.  The reservoir sample of a region with more than
 * MAX_READS_IN_REGION reads is drawn on the device when pa_encoder_set_sampling has switched it on (region_reads[r] is then
 * the count after sampling); without it such a region is the caller's business (the per-region entry points).
 * PA_ERR_UNSUPPORTED: a batch this form does not take (an operation of 2^24 bases, a read that keeps more than 2 L + 64 bases
 * of a region of L positions): nothing was produced, take the host-clipped form.
 * ------------------------------------------------------------------------------------------ */
int pa_polish_chain_run(pa_encoder* e, int32_t n_regions, const pa_packed_region* regions, const uint8_t* arena, int64_t arena_bytes,
                        const pa_packed_read* reads, int32_t n_reads, const int32_t* pair_read, const int32_t* region_pairs,
                        int32_t realign, int32_t chunk_size, int32_t chunk_overlap, int64_t* n_rows, int32_t* region_reads,
                        int32_t* n_chunks, int64_t* total_chunks);
/* The chunks of the last run, region after region, in page-locked memory of the handle (valid until its next run):
 * images uint8 [total_chunks, chunk_size, 10], position / index int64 [total_chunks, chunk_size]. */
int pa_polish_chain_chunks(pa_encoder* e, const uint8_t** images, const int64_t** position, const int64_t** index);
/* The same images where the chunk kernel left them ON THE DEVICE ([total_chunks, chunk_size, 10] uint8, complete when
 * pa_polish_chain_run has returned, valid until the handle's next run): what the polish model reads without the HDF5 round trip
 * (pa_polish_predict_device; pepper_amd/polish/fused.py). */
int pa_polish_chain_device_chunks(pa_encoder* e, const uint8_t** images);
/* Host-clock times of the last run in ms: [0] tables + upload + unpack launch, [1] re-aligner (its waits included) + apply,
 * [2] summary encoder (its wait included), [3] chunk kernel + download; HIP events: [5] score kernels, [6] band launches.
 * counts: [0] (read, region) pairs, [1] reads re-aligned, [2] CIGAR operations written, [3] summary rows, [4] reads whose 8-bit
 * score pass was proven to overflow from their BAM alignment and skipped (ssw.c:819-824 discards that pass's results). */
int pa_polish_chain_last_timing(pa_encoder* e, double* ms, int32_t n_ms, int64_t* counts, int32_t n_counts);

/* ------------------------------------------------------------------------------------------
 * The polish stitch ON THE DEVICE (opt-in: polish(..., device_stitch=True); pepper_amd/csrc/stitch.hip).
 * replaces, for such a run: Stitch.py small_chunk_stitch (:36-94) -- per piece a dictionary keyed (position, insert index),
 * written in loop order, the last write wins, keys in order, gaps dropped.  The piece and loop order of every region
 * (create_consensus_sequence :97-128) stay the caller's: pepper_amd/polish/DeviceStitch.py plan().
 *
 * A handle collects prediction rows while a run goes on (add) and merges one contig at a time at its end (finish, take).
 * Calls on one handle exclude each other; all of them return when their device work is done.
 * ------------------------------------------------------------------------------------------ */
typedef struct pa_stitcher pa_stitcher;

int pa_stitcher_create(int32_t device, void* hip_stream, pa_stitcher** out);
void pa_stitcher_destroy(pa_stitcher* s);
/* out[0] largest position, [1] largest insert index a kept row may have, [2] elements one workgroup of the scans takes,
 * [3] packed rows per slab (the most one chunk may keep). */
int pa_stitcher_limits(int64_t* out, int32_t n);
/* n_chunks chunks of chunk_len rows each of contig `contig` (an id of the caller's): position / index host int64
 * [n_chunks, chunk_len]; labels uint8 [n_chunks, chunk_len], in the memory of the handle's device and complete
 * (labels_on_device != 0) or on the host; per chunk the caller's region id, a value that orders the chunks of a region as the
 * reference iterates them (its ids as strings; equal values keep the order they arrive in) and drop_below: rows with
 * position <= drop_below are the region's overlap and dropped (start + 2 * MIN_IMAGE_OVERLAP for a region with start > 0,
 * else -1).  Rows with a negative position or index are dropped.  Kept rows are packed (8 bytes) behind those of earlier calls.
 * PA_ERR_UNSUPPORTED: a kept row lies beyond the limits, or a chunk keeps more rows than a slab holds; PA_ERR_HIP: no memory
 * for another slab.  A call that fails has added nothing and leaves the handle as it was. */
int pa_stitcher_add(pa_stitcher* s, int32_t contig, int32_t n_chunks, int32_t chunk_len, const int64_t* position, const int64_t* index,
                    const uint8_t* labels, int32_t labels_on_device, const int32_t* region, const int64_t* chunk_order,
                    const int64_t* drop_below);
/* pa_stitcher_add with the rows' qualities: phred uint8 [n_chunks, chunk_len] lies where labels lies (labels_on_device governs
 * both).  A kept row carries its phred in the top byte of its packed word (rows added through pa_stitcher_add carry 0 there);
 * the row that supplies a letter's label supplies its quality.  Qualities are not switched on anywhere: a finish produces them
 * whenever EVERY chunk it merges was added through this entry point (a contig without chunks has them, empty). */
int pa_stitcher_add_qual(pa_stitcher* s, int32_t contig, int32_t n_chunks, int32_t chunk_len, const int64_t* position,
                         const int64_t* index, const uint8_t* labels, const uint8_t* phred, int32_t labels_on_device,
                         const int32_t* region, const int64_t* chunk_order, const int64_t* drop_below);
/* Merge what the handle holds of `contig`: per region id its piece (0 .. n_pieces - 1) and its rank in the loop order.
 * piece_first / piece_last / piece_length [n_pieces]: first and last kept position (-1, -1 for a piece without kept rows) and
 * letters of every piece; *sequence_length letters in all, the pieces ordered by (first, last) as take() copies them.
 * *bad_label != 0: a surviving label that is no base (the reference's label_decoder raises KeyError); no sequence then.
 * The handle keeps the rows: a contig may be finished again, with another plan.
 * PA_ERR_UNSUPPORTED, before any launch: the contig keeps more than 2^48 - 1 rows (the rank's share of the 64-bit word
 * (rank + 1) << 16 | phred << 8 | label that decides a key's last write). */
int pa_stitcher_finish(pa_stitcher* s, int32_t contig, int32_t n_regions, const int32_t* region, const int32_t* piece, const int64_t* rank,
                       int32_t n_pieces, int64_t* piece_first, int64_t* piece_last, int64_t* piece_length, int64_t* sequence_length,
                       int32_t* bad_label);
/* The sequence of the last finish (capacity >= its length; no terminator). */
int pa_stitcher_take(pa_stitcher* s, char* dst, int64_t capacity);
/* The qualities of the last finish, one per letter of pa_stitcher_take and in its order: Sanger text, '!' + min(phred, 93) of
 * the row whose label the letter is (capacity >= the sequence length; no terminator).  PA_ERR_INVALID: no finish yet; the last
 * finish produced no sequence (a bad label, a failure); a chunk of its contig was added without qualities; capacity is short.
 * The handle stays usable. */
int pa_stitcher_take_qualities(pa_stitcher* s, char* dst, int64_t capacity);
/* out[0] rows held, [1] bytes of slabs, and of the last finish: [2] slots, [3] pieces, [4] positions spanned, [5] bytes of
 * its tables (the quality buffer among them when the finish produced qualities, the edit records once pa_stitcher_edits ran,
 * once pa_stitcher_fill ran its table of 4 bytes per position, the filled sequence and the filled qualities, and once
 * pa_stitcher_gate ran its withheld records, and once pa_stitcher_variants ran its tables -- 4 bytes per edit record, 69 per
 * hunk -- and its records). */
int pa_stitcher_stats(pa_stitcher* s, int64_t* out, int32_t n);

/* What the last finish changed against the draft (opt-in, not in the reference; pepper_amd/polish/Edits.py is the host twin and
 * writes the text).  Pieces in take() order, inside a piece the keys (position, insert index) in order; one record for
 *   SUB        slot (p, 0)      the winner is a base and differs from upper(draft[p]) (a draft letter outside ACGT always does)
 *   DEL        slot (p, 0)      the winner is a gap, or the slot has no writer
 *   INS        slot (p, i > 0)  the winner is a base
 *   GAP_OPEN   position p inside the piece without a slot, p - 1 has one
 *   GAP_CLOSE  position p inside the piece without a slot, p + 1 has one (a run of one position: both, GAP_OPEN first)
 * offset counts letters of pa_stitcher_take: the record's own letter for SUB and INS, the letters in front of it otherwise. */
enum { PA_EDIT_SUB = 1, PA_EDIT_DEL = 2, PA_EDIT_INS = 3, PA_EDIT_GAP_OPEN = 4, PA_EDIT_GAP_CLOSE = 5 };
typedef struct pa_stitch_edit {
    uint32_t position;   /* of the draft */
    uint32_t offset;     /* of the consensus */
    uint16_t index;      /* insert index */
    uint16_t piece;      /* the piece's place in take() order */
    uint8_t kind;        /* PA_EDIT_* */
    uint8_t draft;       /* the draft letter upper-cased; 0 for INS */
    uint8_t letter;      /* A, C, G or T; 0 for DEL and the GAP kinds */
    uint8_t phred;       /* the winner's raw phred; 0 without a winner, for the GAP kinds, and for a contig without qualities */
} pa_stitch_edit;        /* 16 bytes */
/* Compare the tables of the last finish with draft[0 .. draft_length): *n_edits records, counts[k] of kind k (counts[0] = 0).
 * One wait; the records stay on the device until pa_stitcher_take_edits, in a buffer allocated on first use and counted in
 * pa_stitcher_stats [5] from then on.  A later finish invalidates them.
 * PA_ERR_INVALID before any launch: no finish yet; the last finish gave no sequence (a bad label, a failure); draft_length <=
 * the largest piece_last; the finish had more than 65 535 pieces; draft is NULL and neither a pa_stitcher_fill nor a
 * pa_stitcher_gate of a draft of draft_length letters ran since the finish.  The handle stays usable. */
int pa_stitcher_edits(pa_stitcher* s, const char* draft, int64_t draft_length, int64_t* n_edits, int64_t* counts /* [6] */);
/* The records of the last pa_stitcher_edits (capacity >= *n_edits records).  PA_ERR_INVALID: pa_stitcher_edits has not run since
 * the last finish; capacity is short.  The handle stays usable. */
int pa_stitcher_take_edits(pa_stitcher* s, pa_stitch_edit* dst, int64_t capacity);

/* Complete the consensus of the last finish with draft[0 .. draft_length), the whole contig of the draft (opt-in, not in the
 * reference; Stitch.py filled_piece is the host twin).  The finish must have had ONE piece (every region in piece 0: the merge
 * of the whole contig).  Every position of the draft without a slot -- in front of the piece's first position, behind its last,
 * and in the runs inside -- gives draft[p] as it is passed (no case folding) with quality '!'; a position with a slot gives what
 * it gave.  *filled_length letters; counts[0] runs filled (the two ends count when they are not empty), counts[1] letters filled.
 * A finish without a kept row is filled with the whole draft.
 * From then on, until the next finish, the handle speaks of the FILLED consensus: pa_stitcher_take and pa_stitcher_take_qualities
 * copy it (capacity >= *filled_length), and pa_stitcher_edits gives its records -- `offset` counts its letters, and a GAP pair's
 * offset is the first filled letter of its run.  Records made before the fill are dropped: pa_stitcher_edits has to run again.
 * That call may pass draft = NULL with the same draft_length: it then reads the copy this call uploaded, so a contig's draft goes
 * to the device once.
 * One wait; one scan over the positions and one lane per position, the ends are copies on the device.
 * PA_ERR_INVALID before any launch: no finish yet; the last finish gave no sequence; it had more than one piece; draft_length <=
 * the piece's last position.  PA_ERR_UNSUPPORTED: the draft or the filled consensus has more than 2^32 - 1 letters.  The handle
 * stays usable, and a refused call changes nothing. */
int pa_stitcher_fill(pa_stitcher* s, const char* draft, int64_t draft_length, int64_t* filled_length, int64_t* counts /* [2] */);

/* Apply only the edits the model is sure of (opt-in, not in the reference; Stitch.py gate_numpy is the host twin).  Runs after a
 * finish with any number of pieces and BEFORE pa_stitcher_fill and pa_stitcher_edits, over the winners of the merge (so the result
 * does not depend on how the rows were chunked or in which order they were added); draft[0 .. draft_length) is the whole contig.
 * With d = upper(draft[p]) and the winner's raw phred (0 for a slot without a writer):
 *   slot (p, 0), d in ACGT, the winner is a base other than d (SUB) or a gap / no writer (DEL), phred < min_phred:
 *       WITHHELD -- the slot emits d, upper-cased, with phred 0 (quality '!')
 *   slot (p, i > 0), the winner is a base (INS), phred < min_phred:   WITHHELD -- the slot emits nothing
 *   everything else -- phred >= min_phred, a winner equal to d, a gap in an insert slot, and EVERY slot (p, 0) whose draft letter
 *   is not one of ACGT -- stays as the model decided it.
 * A withheld slot's letter and winner word are rewritten (phred byte 0, the label of what it emits), the letters are scanned and
 * emitted again: piece_length [n_pieces of the finish] and *sequence_length are those of the gated consensus, and from then on,
 * until the next finish, pa_stitcher_take, _take_qualities, _fill, _edits and _stats speak of it -- the edit records are exactly the
 * applied edits.  A following pa_stitcher_fill or pa_stitcher_edits may pass draft = NULL with the same draft_length and read the
 * copy this call uploaded.  counts: withheld in all, SUB, DEL, INS.  One wait.  The handle keeps its rows: a second finish of the
 * contig gives the ungated tables again.
 * The withheld records (pa_stitcher_take_withheld; capacity >= counts[0]) are pa_stitch_edit-shaped and ordered as the edit records
 * are: kind SUB / DEL / INS, letter the model's (0 for DEL), draft d (0 for INS), phred the winner's, offset the place of the kept
 * draft letter (SUB, DEL) or the letters in front of the slot (INS) in the consensus the handle speaks of when they are taken: the
 * gated one, and after a pa_stitcher_fill the filled one.  They stay on the device until taken; pa_stitcher_stats [5] grows by 16
 * bytes per record, and by the letters the sequence gained or lost (its quality buffer).
 * PA_ERR_INVALID before any launch, the handle stays usable and nothing changes: no finish yet; the finish gave no sequence; a chunk
 * of the contig was added without qualities; draft_length <= the largest piece_last; min_phred outside 1..255; a gate or a fill
 * already ran since the finish; the finish had more than 65 535 pieces; take_withheld without a gate, or with short capacity. */
int pa_stitcher_gate(pa_stitcher* s, const char* draft, int64_t draft_length, int32_t min_phred, int64_t* piece_length,
                     int64_t* sequence_length, int64_t* counts /* [4] */);
int pa_stitcher_take_withheld(pa_stitcher* s, pa_stitch_edit* dst, int64_t capacity);

/* What the FILLED consensus changed against the draft as normalised variant records, one per hunk (opt-in, not in the reference;
 * pepper_amd/polish/Variants.py states the rule, records_numpy there is the host twin and lines() writes the VCF text).  Runs
 * after pa_stitcher_fill (and after pa_stitcher_gate where there is one); draft = NULL reads the copy the fill uploaded.  Where the
 * edit records of the filled consensus are not there yet the call makes them as pa_stitcher_edits does (they can be taken).
 *
 * THE RULE.  The units are runs of SUB / DEL / INS edit records: a record joins its predecessor when its draft interval and its
 * consensus interval begin where the predecessor's end (SUB [p, p+1) [o, o+1); DEL [p, p+1) [o, o); INS [p+1, p+1) [o, o+1)); GAP
 * records join nothing and give nothing.  Hunk i: the draft interval [a0, b0), the letters ALT0 = consensus[o0, o1), q = the
 * minimum phred of its records.  With d = the draft upper-cased:
 *   1. Trim: while both alleles are non-empty and end in the same letter drop it from both, then the same for the first letter:
 *      (a, b, alt).  Both empty: a no-op, no record, counted.  Both non-empty: REF = d[a, b), ALT = alt, at position a.
 *   2. A pure indel (one allele empty) moves left while a - 2 >= bound and d[a-1] == d[b-1] (deletion) or d[a-1] == alt[-1]
 *      (insertion, which rotates: alt = d[a-1] + alt[:-1]); then REF = d[a-1, b), ALT = d[a-1] + alt, at position a - 1.
 *      bound = the UNTRIMMED b0 of the hunk in front, 0 for the first.
 *   3. link_0: hunk 0 is a pure indel with a == 0; link_j: hunk j is a pure indel with a_j == b_(j-1) + 1 (both trimmed).  F = the
 *      first j whose link is false.  Hunks i < F are anchored on the right and not moved: REF = d[a, b+1), ALT = alt + d[b], at
 *      position a; one with b == draft_length has no letter on either side: no record, counted as unanchored.  Hunk F > 0 takes
 *      bound = b_(F-1) + 1.
 * A record carries no letters:  REF = draft[position, position + ref_len);  ALT = draft[position, position + lead), then
 * consensus[offset, offset + alt_len - lead - tail), then for tail = 1 draft[position + ref_len - 1].  A moved insertion of n letters
 * has lead = 1 + min(shift, n), a deletion lead 1, a right-anchored record lead 0 and tail 1, every other record lead 0 and tail 0.
 * Records in hunk order (ascending position, REF intervals disjoint).  Two runs over the same input leave the same bytes. */
enum { PA_VARIANT_SUB = 1, PA_VARIANT_INS = 2, PA_VARIANT_DEL = 3, PA_VARIANT_COMPLEX = 4 };
typedef struct pa_stitch_variant {
    uint32_t position;   /* of the draft, 0-based: where REF begins */
    uint32_t ref_len;
    uint32_t alt_len;
    uint32_t lead;       /* letters of ALT that are the draft's, from `position` on */
    uint32_t offset;     /* of the filled consensus: where the hunk's trimmed letters begin */
    uint32_t shift;      /* places a pure indel moved left */
    uint8_t phred;       /* the minimum over the hunk's edit records; 0 for a contig without qualities */
    uint8_t kind;        /* PA_VARIANT_*, of the trimmed hunk */
    uint8_t tail;        /* 1: anchored on the right, ALT ends in draft[position + ref_len - 1] */
    uint8_t pad;         /* 0 */
    uint32_t reserved;   /* 0 */
} pa_stitch_variant;     /* 32 bytes */
/* *n_variants records; counts: records, no-ops, unanchored, hunks moved, places moved in all.  One wait for the hunks, one for the
 * records; the records stay on the device until pa_stitcher_take_variants, in buffers counted in pa_stitcher_stats [5] from then on.
 * A later finish, gate or fill invalidates them.
 * PA_ERR_INVALID before any launch, the handle stays usable: no finish yet; the last finish gave no sequence; no pa_stitcher_fill
 * since the finish; draft_length is not the fill's; draft is NULL and the fill's copy is gone (a pa_stitcher_edits with a draft of
 * its own replaced it); take_variants without a run since the last finish, or with short capacity. */
int pa_stitcher_variants(pa_stitcher* s, const char* draft, int64_t draft_length, int64_t* n_variants, int64_t* counts /* [5] */);
int pa_stitcher_take_variants(pa_stitcher* s, pa_stitch_variant* dst, int64_t capacity);

/* ------------------------------------------------------------------------------------------
 * The candidate finder's selection ON THE DEVICE (opt-in: call_variant(..., fused_inference=True, device_selection=True);
 * pepper_amd/csrc/select.hip).
 * replaces, for such a run: which rows of a prediction batch pa_candidates_reference_flags + pa_candidates_select_format
 * (include/pepper_amd_io.h; CandidateFinder.py:356-581) keep, decided where the encoder left the lists and the model the
 * probabilities.  Only the kept rows come back, compacted in row order; their record TEXT (%g, round(x, 3),
 * int(-10 log10(..)), the QUAL cutoff of flags bit 1) stays with pa_candidates_select_format on the host, which is handed
 * the compacted arrays and keeps all of them.
 *
 * A row is kept exactly when the host pair keeps it: the reference letter ref[p] upper-cased is one of ACGT; the name is a
 * type character followed by letters of ACGT only, and the type is '1'..'3'; non_alt = max(p1, p2) widened to double is
 * >= p_value[kind] (p_value_in_lc[kind] where the low-complexity flag is set), or 0 < report_above_freq[kind] <=
 * (double)support / (double)depth.  The low-complexity flag: a run of at least 5 equal upper-cased letters inside
 * ref[max(0, p - 10), p + 10), cut at the end of the reference given, that shares an index with [p - 5, p + 4).
 * flags: bit 0 SNP (from the swapped lengths), bit 2 REF / ALT swapped (a deletion admitted by probability), bits 4-5 the
 * genotype (first maximum of the three probabilities); bit 1 is not computed here.
 *
 * Handed back instead of decided (summary.status != 0, nothing can be taken; the caller does that call on the host):
 *   PA_SELECT_ZERO_DEPTH   a row with a valid letter and a valid allele has depth 0 (the host path returns -2)
 *   PA_SELECT_NAN          a row that reaches the rules has a NaN probability (the host path returns -2)
 *   PA_SELECT_NAME         a name is empty, longer than pa_selector_limits [2] bytes or holds one of " ,'\"[]\n"
 *   PA_SELECT_CONTEXT      a row inside its reference whose context starts in front of reference[0] while reference_start > 0
 *   PA_SELECT_NAME_COUNT   `names` does not hold exactly n NULs
 * Two runs over the same input leave the same bytes: nothing depends on the order workgroups or atomics run in.
 * ------------------------------------------------------------------------------------------ */
#ifndef PA_CANDIDATE_RULES_DEFINED
#define PA_CANDIDATE_RULES_DEFINED
typedef struct {
    double p_value[3], p_value_in_lc[3], report_above_freq[3];
    double snp_q_cutoff, snp_q_cutoff_in_lc, indel_q_cutoff, indel_q_cutoff_in_lc;
} pa_candidate_rules;
#endif
typedef struct pa_selector pa_selector;
typedef struct {
    int64_t first_row;         /* rows [first_row, next region's first_row) lie in this region; regions[0].first_row = 0 */
    int64_t reference_start;   /* contig coordinate of reference[0] */
    const char* reference;
    int64_t reference_len;
} pa_selector_region;
enum { PA_SELECT_ZERO_DEPTH = 1, PA_SELECT_NAN = 2, PA_SELECT_NAME = 4, PA_SELECT_CONTEXT = 8, PA_SELECT_NAME_COUNT = 16 };
typedef struct {
    int64_t kept_rows;         /* m */
    int64_t kept_name_bytes;   /* bytes of the m kept names, their NULs included */
    int32_t status;            /* 0, or the PA_SELECT_* bits of the cases found */
    int32_t reserved;
} pa_selection;

/* One selector per (thread, stream): owns its workspace; hip_stream NULL: a stream of its own. */
int pa_selector_create(int32_t device, void* hip_stream, pa_selector** out);
void pa_selector_destroy(pa_selector* s);
/* out[0] rows per workgroup, [1] elements one workgroup of the scans takes, [2] longest name taken (bytes without the NUL),
 * [3] the most elements a scan takes without a further level, [4] the most rows of a call. */
int pa_selector_limits(int64_t* out, int32_t n);
/* One call's rows: position int64 [n], depth / support int32 [n], prediction float32 [n, 3], names = n NUL-terminated strings
 * back to back (name_bytes of them, as the encoder leaves them), regions ascending by first_row.  on_device 0: every array
 * (the regions' references too) is host memory and is uploaded; 1: device memory of the selector's device, complete.  One
 * submission on the selector's stream and one wait, for *summary. */
int pa_selector_run(pa_selector* s, const pa_candidate_rules* rules, int64_t n, const int64_t* position, const int32_t* depth,
                    const int32_t* support, const float* prediction, const char* names, int64_t name_bytes, int32_t n_regions,
                    const pa_selector_region* regions, int32_t on_device, pa_selection* summary);
/* The ploidy of the contig the selector's next runs are about (options.haploid_contigs / par_regions_bed;
 * pepper_amd/variant/Ploidy.py).  A call's rows are one contig.  haploid_contig 0 (with n_par 0, NULL, NULL): every row diploid,
 * the state of a new selector.  Otherwise position p is haploid unless par_start[k] <= p < par_end[k] for some k: n_par
 * intervals, 0-based and half-open, ascending and disjoint (HOST pointers; uploaded to the selector's device here, not per run:
 * set it again only when the contig changes).  At a haploid row pa_selector_run and pa_encoder_select_candidates decide from
 * the primed triple,
 *     s   = (double)p0 + (double)p2
 *     p0' = (float)((double)p0 / s),  p1' = 0.0f,  p2' = (float)((double)p2 / s)     if s != 0
 *     p0' = 0.5f,                     p1' = 0.0f,  p2' = 0.5f                         if s == 0
 * exactly where they read the model's: the genotype (first maximum: 0 or 2), non_alt = max(p1', p2') against p_value[_in_lc],
 * the deletion swap.  A NaN in the triple still sets PA_SELECT_NAN; the frequency admission, the low-complexity flag and the
 * letter / name checks do not see the ploidy.  flags bit 3 is set on the haploid rows that are kept.  The compacted prediction
 * stays the MODEL's triple: pa_candidates_select_format_ploidy primes it again from flags bit 3.  A run stays one submission and
 * one wait.  PA_ERR_INVALID: intervals without a haploid contig, or a table that is not ascending and disjoint. */
int pa_selector_set_ploidy(pa_selector* s, int32_t haploid_contig, int64_t n_par, const int64_t* par_start, const int64_t* par_end);
/* The m kept rows of the last run in row order (HOST pointers, any may be NULL): their row numbers, flags, reference letters
 * and low-complexity flags, the compacted fields, the kept names back to back and where each begins (name_offsets[m] = the
 * kept name bytes).  One wait.  PA_ERR_INVALID: no run, or its status was not 0. */
int pa_selector_take(pa_selector* s, int32_t* row, uint8_t* flags, uint8_t* letter, uint8_t* in_repeat, int64_t* position,
                     int64_t* depth, int64_t* support, float* prediction, char* names, int64_t* name_offsets);
/* pa_selector_run over the encoder's last variant run: the lists are read where the device enumeration left them (a
 * host-enumerated run uploads its lists first), the references in the staged batch, a row's region from the run's counts;
 * prediction float32 [n, 3] in device memory, complete.  Nothing is downloaded to set the call up. */
int pa_encoder_select_candidates(pa_encoder* e, pa_selector* s, const float* prediction, const pa_candidate_rules* rules,
                                 pa_selection* summary);

#ifdef __cplusplus
}
#endif
#endif /* PEPPER_AMD_ENCODER_H */
