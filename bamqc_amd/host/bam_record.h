// bam_record.h — what a BAM record IS, stated once for the host reader (bam_io.cpp) and the reader on the card (csrc/gpu_bam.hip), which
// must agree byte for byte: the size rule of the block_size chain, the test "a record may start here", the scan of the optional
// fields (RG, NM, AS) and the flag annotation.  Plain C++17 (g++ alone builds it), host and device code under hipcc.
//
// Every rule is a template over a BYTE SOURCE: any type with u8(o) / u16(o) / u32(o) — little-endian values at the 64-bit offset o
// from the source's origin — and find0(from, end), the offset of the first NUL in [from, end) or `end`.  BrBytes below is the plain
// pointer; the card has two more over bytes it has staged in LDS (gpu_bam.hip: GbwView, GbdStage).
// Record layout, tag types: the public SAM/BAM specification; the rules for RG / NM / AS are the reference's (bamqualcheck.cpp:72-100
// getLane, QualityCheck.hpp:201-209 NM, TripletCounting.hpp:113-127 AS).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/bamqc.h"

#if defined(__HIP__) || defined(__HIPCC__)
#define BR_RULE __host__ __device__ inline __attribute__((always_inline)) // (bam_io.cpp does not include the HIP runtime's header)
#else
#define BR_RULE inline
#endif

struct BrBytes {
    const uint8_t* p;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint16_t __attribute__((aligned(1))) u16_u;
    typedef uint32_t __attribute__((aligned(1))) u32_u;
    BR_RULE uint32_t u16(uint64_t o) const { return *(const u16_u*)(p + o); }
    BR_RULE uint32_t u32(uint64_t o) const { return *(const u32_u*)(p + o); }
    BR_RULE uint64_t find0(uint64_t from, uint64_t end) const { while (from < end && p[from]) ++from; return from; }
#else // (assembled from bytes: no alignment is assumed)
    BR_RULE uint32_t u16(uint64_t o) const { return (uint32_t)(p[o] | (p[o + 1] << 8)); }
    BR_RULE uint32_t u32(uint64_t o) const { return p[o] | (p[o + 1] << 8) | (p[o + 2] << 16) | ((uint32_t)p[o + 3] << 24); }
    BR_RULE uint64_t find0(uint64_t from, uint64_t end) const { const void* z = memchr(p + from, 0, (size_t)(end - from)); return z ? (uint64_t)((const uint8_t*)z - p) : end; }
#endif
    BR_RULE uint32_t u8(uint64_t o) const { return p[o]; }
};

// ---- the record at offset p: block_size (4 bytes), 32 fixed bytes, read name, CIGAR, packed bases, qualities, optional fields -------
struct BrHead { uint32_t bs, l_name, n_cig, l_seq; };
template <class S> BR_RULE BrHead br_head(const S& s, uint64_t p) { return BrHead{s.u32(p), s.u8(p + 12), s.u16(p + 16), s.u32(p + 20)}; }
// bytes of block_size that the fixed part and the four arrays need
BR_RULE uint64_t br_var(const BrHead& h) { return 32ull + h.l_name + 4ull * h.n_cig + ((uint64_t)h.l_seq + 1) / 2 + h.l_seq; }
// where the arrays start, from the record's start (its end is 4 + bs)
BR_RULE uint64_t br_cigar_off(const BrHead& h) { return 36ull + h.l_name; }
BR_RULE uint64_t br_seq_off(const BrHead& h) { return br_cigar_off(h) + 4ull * h.n_cig; }
BR_RULE uint64_t br_qual_off(const BrHead& h) { return br_seq_off(h) + (h.l_seq + 1u) / 2u; }
BR_RULE uint64_t br_tags_off(const BrHead& h) { return br_qual_off(h) + h.l_seq; }

// One step of the block_size chain with `left` bytes of data from the record's start on.  What a walk does with the answer is the
// walk's business (BR_SHORT, a block_size below 32, is a corrupt record like BR_CORRUPT: it has a value of its own because the host
// reader has always reported it in other words).  The test of `left` stays first: with fewer than 36 bytes nobody has read a header,
// and callers pass an h they have not filled (br_step below, the chain loop of k_gb_walk_wave).
enum BrCheck { BR_OK = 0, BR_INCOMPLETE, BR_CORRUPT, BR_SHORT };
BR_RULE BrCheck br_check(const BrHead& h, uint64_t left)
{
    if (left < 36) return BR_INCOMPLETE;
    if (h.bs < 32u) return BR_SHORT;
    if (br_var(h) > h.bs) return BR_CORRUPT;
    return 4ull + h.bs > left ? BR_INCOMPLETE : BR_OK;
}
// br_check of the record at p of `avail` bytes, its header read when it is there
template <class S> BR_RULE BrCheck br_step(const S& s, uint64_t avail, uint64_t p, BrHead& h)
{
    h = p + 36 <= avail ? br_head(s, p) : BrHead{0, 0, 0, 0};
    return br_check(h, avail > p ? avail - p : 0);
}

// "A record may start at p": what a walk that does not know where the chain arrives tests, three records in a row (how a chain
// that runs off the data counts is the caller's rule).  next: where the following record starts.
template <class S> BR_RULE bool br_plausible(const S& s, uint64_t avail, uint64_t p, int32_t n_ref, uint64_t& next)
{
    if (p + 36 > avail) return false;
    const uint32_t bs = s.u32(p);
    if (bs < 32u || bs > (1u << 28)) return false;
    const int32_t rid = (int32_t)s.u32(p + 4), pos = (int32_t)s.u32(p + 8), rnext = (int32_t)s.u32(p + 24), pnext = (int32_t)s.u32(p + 28);
    if (rid < -1 || rid >= n_ref || rnext < -1 || rnext >= n_ref || pos < -1 || pnext < -1) return false;
    const BrHead h = br_head(s, p);
    if (h.l_name == 0 || h.l_seq > (1u << 28)) return false;
    if (br_var(h) > bs) return false;
    if (p + br_cigar_off(h) <= avail && s.u8(p + br_cigar_off(h) - 1) != 0) return false; // read name is NUL-terminated
    next = p + 4 + bs;
    return true;
}

// ---- optional fields --------------------------------------------------------------------------------------------------------------
enum { BR_TAGS_CORRUPT = 1, BR_RG_SEEN = 2, BR_RG_NOT_Z = 4, BR_NM_SEEN = 8 };
struct BrTags {
    int32_t nm, as;          // first integer NM, first AS (BQC_NM_ABSENT / BQC_AS_ABSENT)
    uint32_t flags;          // BR_*
    uint32_t rg_len;         // the first RG:Z value without its NUL, at rg_off of the source: which lane that is, is the caller's table
    uint64_t rg_off;
};
// One linear scan of the `len` bytes of optional fields at the source's origin: the first RG, every integer NM (the first is the
// read's value, each further one goes to on_extra_nm), the first AS.  A field that does not fit ends the scan (BR_TAGS_CORRUPT).
template <class S, class F> BR_RULE BrTags br_scan_tags(const S& s, uint64_t len, F&& on_extra_nm)
{
    BrTags T{BQC_NM_ABSENT, BQC_AS_ABSENT, 0, 0, 0};
    bool as_seen = false;
    for (uint64_t tg = 0; tg + 3 <= len;) {
        const char k0 = (char)s.u8(tg), k1 = (char)s.u8(tg + 1), ty = (char)s.u8(tg + 2);
        const uint64_t v = tg + 3;
        uint64_t n = 0; // bytes of the value
        switch (ty) {
        case 'A': case 'c': case 'C': n = 1; break;
        case 's': case 'S': n = 2; break;
        case 'i': case 'I': case 'f': n = 4; break;
        case 'Z': case 'H': { const uint64_t z = s.find0(v, len); n = z < len ? z - v + 1 : len - v; break; }
        case 'B': {
            if (v + 5 > len) { n = len - v; break; }
            const char st = (char)s.u8(v);
            n = 5 + (uint64_t)s.u32(v + 1) * ((st == 'c' || st == 'C') ? 1u : (st == 's' || st == 'S') ? 2u : 4u);
            break;
        }
        default: n = len - v; break;
        }
        if (n > len - v) { T.flags |= BR_TAGS_CORRUPT; break; }
        if (k0 == 'R' && k1 == 'G' && !(T.flags & BR_RG_SEEN)) {
            T.flags |= BR_RG_SEEN;
            if (ty == 'Z') { T.rg_off = v; T.rg_len = n ? (uint32_t)n - 1 : 0; }
            else T.flags |= BR_RG_NOT_Z;
        } else if (k0 == 'N' && k1 == 'M' && (ty == 'c' || ty == 'C' || ty == 's' || ty == 'S' || ty == 'i' || ty == 'I')) {
            uint32_t x;
            switch (ty) {
            case 'c': x = (uint32_t)(int32_t)(int8_t)s.u8(v); break;
            case 'C': x = s.u8(v); break;
            case 's': x = (uint32_t)(int32_t)(int16_t)s.u16(v); break;
            case 'S': x = s.u16(v); break;
            default: x = s.u32(v); break;
            }
            if (!(T.flags & BR_NM_SEEN)) { T.nm = (int32_t)x; T.flags |= BR_NM_SEEN; }
            else on_extra_nm((int32_t)x);
        } else if (k0 == 'A' && k1 == 'S' && !as_seen) {
            as_seen = true;
            switch (ty) {
            case 'A': T.as = (int32_t)(char)s.u8(v); break;
            case 'c': T.as = (int8_t)s.u8(v); break;
            case 'C': T.as = (int32_t)s.u8(v); break;
            case 's': T.as = (int16_t)s.u16(v); break;
            case 'S': T.as = (int32_t)s.u16(v); break;
            case 'i': case 'I': T.as = (int32_t)s.u32(v); break;
            case 'f': { const uint32_t u = s.u32(v); float f; __builtin_memcpy(&f, &u, 4); T.as = (int32_t)f; break; }
            default: T.as = BQC_AS_ABSENT; break; // extractTagValue fails -> "Could not read AS tag"
            }
        }
        tg = v + n;
    }
    return T;
}

// the flag column: the record's twelve flag bits and the decoder's two annotations (first_qual: the first quality byte; any value when l_seq is 0)
BR_RULE uint32_t br_flag(uint32_t flag, int32_t rnext, const uint8_t* main_chrom, uint64_t n_main, uint32_t l_seq, uint32_t first_qual)
{
    uint32_t f = flag & 0x0FFFu;
    if (rnext >= 0 && (uint64_t)rnext < n_main && main_chrom[rnext]) f |= BQC_FLAG_MATE_MAIN;
    if (l_seq > 0 && first_qual == 0xFF) f |= BQC_FLAG_NO_QUAL;
    return f;
}
