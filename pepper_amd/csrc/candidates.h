// The order of a site's alleles and the rule that makes one a candidate, written once for the host enumeration
// (encoder.hip: enumerate_region) and the device enumeration (encoder.hip: enumerate_sites_kernel).  Plain inline functions,
// no HIP types, no library calls: g++ and hipcc (host and device pass) all compile this file, so the two enumerations cannot
// drift apart.
//
// What it restates (the reference's region_summary.cpp:667-916): per passing site a std::set<std::string> of allele keys --
// "1" + base, "2" + anchor + inserted bases, "3" + deleted reference bases -- walked in the set's order; a key becomes a
// candidate when its support and its frequency (in double) reach the thresholds and its type passed at the site.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PA_CD_FN __host__ __device__ inline
#else
#define PA_CD_FN inline
#endif

namespace pa_cand {

constexpr int MAXC = 125;           // the int8 clamp of depth, frequency, strand depths and allele length
constexpr int POOL_SLOT = 64;       // bytes per pooled allele (an allele is at most 61 bytes, region_summary.cpp:455)
constexpr int SNP_MAX = 4 + 12;     // SNP alleles one site can hold: A C G T and twelve letters of the rare alphabet

struct SiteRec { int32_t region, idx, cov, flags, fwd[4], rev[4]; };
// meta = type (1 insert, 2 delete) | reverse << 2 | from_ref << 3 | len << 4 | region << 10; prefix = the first 8 bytes of the allele,
// first byte in the top bits (compares like the string), filled for the votes of passing rows: alleles are ordered without touching
// the reads unless two of them agree on 8 bytes
struct Vote { uint32_t idx, meta; int64_t off; uint64_t prefix; };
struct CandDesc {
    int32_t idx, type;        // row of the candidate site; 1 SNP, 2 insert, 3 delete
    int32_t vcol, vval;       // columns 1/2/3 <- alt base code / allele length
    int32_t fwd, rev;         // strand allele depths (<= 125) for columns 5..7 / 16..18
    int32_t neg_f, neg_r;     // columns negated on the centre row (-1: none)
    int32_t last;             // delete: last spill row of the window (else -1)
    int32_t star_f, star_r;   // delete: '*' columns negated on spill rows
    int32_t region;
};
struct Tally { int total, fwd, rev; };      // (no initialisers: it lives in LDS too)
struct SnpAllele { char base; Tally t; };
// what the rule needs of a region's parameters (pa_summary_params) and its pileup
struct Rule {
    double support, snp_freq, indel_freq;     // candidate_support_threshold, snp_ / indel_candidate_freq_threshold
    int64_t region_start;
    int32_t skip_indels;
    int32_t last_cap;                         // candidate_window_size - 1: the last row a deletion may spill to
};

PA_CD_FN bool is_acgt(char c) {
    c &= ~0x20;
    return c == 'A' || c == 'C' || c == 'G' || c == 'T';
}
PA_CD_FN int up(char c) { return (c >= 'a' && c <= 'z') ? c - 32 : c; }
// column of `symbol` for a strand, -1 if the reference base is not A/C/G/T (region_summary.cpp:201-230)
PA_CD_FN int symbol_column(char ref_base, char symbol, bool reverse) {
    if (!is_acgt(ref_base)) return -1;
    const int first = reverse ? 19 : 8;
    switch (up(symbol)) {
        case 'A': return first;
        case 'C': return first + 1;
        case 'G': return first + 2;
        case 'T': return first + 3;
        case 'I': return first + 4;
        case 'D': return first + 5;
        default: return first + 6;
    }
}
PA_CD_FN int base_code(char c) {
    switch (up(c)) {
        case 'A': return 1;
        case 'C': return 2;
        case 'G': return 3;
        case 'T': return 4;
        default: return 5;
    }
}
PA_CD_FN int clamp_count(int v) { return v < MAXC ? v : MAXC; }

// ---- the order ------------------------------------------------------------------------------------------------------
// where the bytes of a vote's allele past the first eight live: deleted bases in the region's reference, inserted ones in the
// pool slot pack_results_kernel filled (the first eight are the vote's prefix)
struct AlleleSrc { const char* reference; const char* pool; };
PA_CD_FN uint32_t allele_len(const Vote& v) { return (v.meta >> 4) & 63u; }
PA_CD_FN const char* allele_tail(const Vote& v, const AlleleSrc& p) {
    return ((v.meta & 8u) ? p.reference + v.off : p.pool + (size_t)v.off * POOL_SLOT) + 8;
}
// memcmp: bytes as unsigned chars
PA_CD_FN int bytes_cmp(const char* x, const char* y, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k) {
        const unsigned char a = (unsigned char)x[k], b = (unsigned char)y[k];
        if (a != b) return a < b ? -1 : 1;
    }
    return 0;
}
// order of the votes of one region: site, then the allele key as std::map<std::string> orders "2..." / "3..." strings
// (type character, bytes as unsigned chars, the shorter of two that agree first).  The 8-byte prefix decides nearly always.
PA_CD_FN bool vote_less(const Vote& x, const Vote& y, const AlleleSrc& p) {
    if (x.idx != y.idx) return x.idx < y.idx;
    const uint32_t tx = x.meta & 3u, ty = y.meta & 3u;
    if (tx != ty) return tx < ty;
    if (x.prefix != y.prefix) return x.prefix < y.prefix;
    const uint32_t lx = allele_len(x), ly = allele_len(y);
    if (lx > 8 && ly > 8) {
        const int c = bytes_cmp(allele_tail(x, p), allele_tail(y, p), (lx < ly ? lx : ly) - 8);
        if (c != 0) return c < 0;
    }
    return lx < ly;
}
PA_CD_FN bool same_allele(const Vote& x, const Vote& y, const AlleleSrc& p) {
    if (x.idx != y.idx || ((x.meta ^ y.meta) & 3u) || x.prefix != y.prefix) return false;
    const uint32_t lx = allele_len(x), ly = allele_len(y);
    return lx == ly && (lx <= 8 || bytes_cmp(allele_tail(x, p), allele_tail(y, p), lx - 8) == 0);
}
// the allele's bytes, `len` of them, to out (the key without its type character)
PA_CD_FN void copy_allele(char* out, const Vote& v, const AlleleSrc& p) {
    const uint32_t len = allele_len(v);
    for (uint32_t k = 0; k < (len < 8u ? len : 8u); ++k) out[k] = (char)(v.prefix >> (56 - 8 * k));
    if (len > 8) {
        const char* tail = allele_tail(v, p);
        for (uint32_t k = 8; k < len; ++k) out[k] = tail[k - 8];
    }
}

// ---- SNP alleles of a site, ordered by the raw base character ---------------------------------------------------------
// A C G T from the site's tallies (already in that order)
PA_CD_FN int snp_from_site(const SiteRec& s, SnpAllele* snp) {
    const char acgt[4] = {'A', 'C', 'G', 'T'};
    int n = 0;
    for (int k = 0; k < 4; ++k)
        if (s.fwd[k] + s.rev[k] > 0) {
            snp[n].base = acgt[k];
            snp[n].t.total = s.fwd[k] + s.rev[k];
            snp[n].t.fwd = s.fwd[k];
            snp[n].t.rev = s.rev[k];
            ++n;
        }
    return n;
}
// tallies of one letter of the rare alphabet added to the site's alleles; false: the letter is new and the site is full
// (more than 12 distinct non-ACGT read letters at one site: not a pileup)
PA_CD_FN bool snp_merge(SnpAllele* snp, int& n, char base, int total, int fwd, int rev) {
    int at = 0;
    while (at < n && snp[at].base != base) ++at;
    if (at == n) {
        if (n == SNP_MAX) return false;
        snp[n].base = base;
        snp[n].t.total = snp[n].t.fwd = snp[n].t.rev = 0;
        ++n;
    }
    snp[at].t.total += total;
    snp[at].t.fwd += fwd;
    snp[at].t.rev += rev;
    return true;
}
PA_CD_FN void snp_sort(SnpAllele* snp, int n) {
    for (int i = 1; i < n; ++i) {
        const SnpAllele x = snp[i];
        int j = i;
        for (; j > 0 && x.base < snp[j - 1].base; --j) snp[j] = snp[j - 1];
        snp[j] = x;
    }
}

// ---- the rule ----------------------------------------------------------------------------------------------------------
// type 1 SNP, 2 insert, 3 delete; depth = min(coverage, 125); flags = the site's pass flags (1 SNP, 2 insert, 4 delete).
// The frequency is an IEEE double quotient compared in double, as the reference computes it.
PA_CD_FN bool accepted(int type, const Tally& t, int depth, int flags, const Rule& q) {
    const double d = (double)depth;
    const double freq = (double)t.total / (d > 1.0 ? d : 1.0);
    if ((double)t.total < q.support) return false;
    if (type != 1 && freq < q.indel_freq) return false;
    if (type == 1 && freq < q.snp_freq) return false;
    if (type != 1 && q.skip_indels) return false;
    if ((type == 1 && !(flags & 1)) || (type == 2 && !(flags & 2)) || (type == 3 && !(flags & 4))) return false;
    return true;
}
// rb = the reference base at the site ('N' outside the reference)
PA_CD_FN CandDesc snp_desc(int32_t region, int32_t idx, char rb, char base, const Tally& t) {
    CandDesc d;
    d.idx = idx; d.type = 1; d.vcol = 1; d.vval = base_code(base);
    d.fwd = clamp_count(t.fwd); d.rev = clamp_count(t.rev);
    d.neg_f = symbol_column(rb, base, false); d.neg_r = symbol_column(rb, base, true);
    d.last = -1; d.star_f = d.star_r = -1;
    d.region = region;
    return d;
}
// type 2 insert / 3 delete of `alen` allele bytes; mid = the window's centre row
PA_CD_FN CandDesc indel_desc(int32_t region, int32_t idx, char rb, int type, int alen, const Tally& t, int mid, const Rule& q) {
    CandDesc d;
    d.idx = idx; d.type = type;
    d.fwd = clamp_count(t.fwd); d.rev = clamp_count(t.rev);
    d.vval = clamp_count(alen);
    d.star_f = d.star_r = -1;
    if (type == 2) {
        d.vcol = 2; d.last = -1;
        d.neg_f = symbol_column(rb, 'I', false); d.neg_r = symbol_column(rb, 'I', true);
    } else {
        d.vcol = 3; d.last = mid + alen - 1 < q.last_cap ? mid + alen - 1 : q.last_cap;
        d.neg_f = symbol_column(rb, 'D', false); d.neg_r = symbol_column(rb, 'D', true);
        d.star_f = symbol_column(rb, '*', false); d.star_r = symbol_column(rb, '*', true);
    }
    d.region = region;
    return d;
}

}  // namespace pa_cand
