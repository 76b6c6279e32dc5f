// The per-record decisions of the packed walk over record headers, written once for the host (bamio.cpp: pack_walk, behind
// pa_bam_pack_headers) and the device (encoder.hip: pack_scan_kernel, behind pa_encoder_pack_records).  Plain inline
// functions, no HIP types: g++ and hipcc both compile this file.
//
// What it restates (the iterator and filters of the reference's get_reads, bam_handler.cpp:138-151, over a run of regions
// whose starts and stops both ascend):
//     a header of a later contig, of no contig, or at / beyond the last stop ends the walk; one of an earlier contig is skipped
//     a record is dropped by its flags, its mapping quality, or when it has no bases / no operations
//     a kept record at `pos` covering ref_len reference bases is a read of the regions r with stop[r] > pos and
//     start[r] < pos + max(1, ref_len): one contiguous run
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PA_PK_FN __host__ __device__ inline
#else
#define PA_PK_FN inline
#endif

namespace pa_pack {

enum { HDR_SKIP = 0, HDR_STOP = 1, HDR_CONTIG = 2 };

// what a header means to the walk over contig `tid`
PA_PK_FN int header_class(int32_t ref_id, int64_t pos, int32_t tid, int64_t last_stop) {
    if (ref_id != tid) return (ref_id > tid || ref_id < 0) ? HDR_STOP : HDR_SKIP;
    return pos >= last_stop ? HDR_STOP : HDR_CONTIG;
}

// the filters: flag = the BAM flag word, l_seq / n_cigar as the record (or its CG tag) gives them
PA_PK_FN bool record_dropped(uint32_t flag, int32_t mapq, uint32_t l_seq, uint32_t n_cigar, int32_t include_supplementary,
                             int32_t min_mapq) {
    if (flag & (0x200u | 0x400u | 0x100u | 0x4u)) return true;
    if (!include_supplementary && (flag & 0x800u)) return true;
    if (mapq < min_mapq) return true;
    return l_seq == 0 || n_cigar == 0;
}

// the first region whose stop lies beyond pos: the regions in front of it can get no read from a record at pos or later
PA_PK_FN int32_t first_open_region(const int64_t* stop, int32_t n_regions, int64_t pos) {
    int32_t lo = 0, hi = n_regions;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (stop[mid] <= pos) lo = mid + 1; else hi = mid;
    }
    return lo;
}

PA_PK_FN int64_t read_end(int64_t pos, int64_t ref_len) { return pos + (ref_len > 1 ? ref_len : 1); }

// one past the last region of a read that ends at `end` and whose first open region is r_lo: r_lo <= r, start[r] < end
PA_PK_FN int32_t region_range_end(const int64_t* start, int32_t n_regions, int32_t r_lo, int64_t end) {
    int32_t lo = r_lo, hi = n_regions;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (start[mid] < end) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// bytes of a kept record's slice(s): operations, 4-bit bases, qualities
PA_PK_FN int64_t slice_bytes(uint32_t n_cigar, uint32_t l_seq) { return 4ll * n_cigar + (l_seq + 1) / 2 + l_seq; }

// bytes a (read, region) pair gets for n clipped bases in the byte-per-base arrays: unpack_clip_kernel decodes four bases per
// store, and a pair's first base sits on a multiple of 4
PA_PK_FN int64_t base_room(int64_t n_bases) { return ((n_bases + 3) & ~(int64_t)3) + 4; }

}  // namespace pa_pack
