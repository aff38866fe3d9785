// mbc_walk.h — what k_mbc.hip and k_sbc.hip share: a thread's walk over the CIGAR of its read (every match-like operation becomes a
// run of stored positions, cut to the read, to the contig and to the cycles below N) and the loads of bytes that start anywhere as
// aligned dwords.  The mapping these serve is described in k_mbc.hip.
#pragma once
#include "kernels_common.h"

// the bytes at the addresses [a_lo, a_hi] (a_hi - a_lo <= 4) as the one or two aligned dwords that hold them, the dword of a_lo lowest.
// Only dwords that hold one of those bytes are touched: such a dword lies in the page of that byte.
__device__ __forceinline__ uint64_t mb_load(uintptr_t a_lo, uintptr_t a_hi)
{
    const gmem_u32* a = (const gmem_u32*)(a_lo & ~(uintptr_t)3); // (global, said so: through the integer the compiler sees a flat pointer)
    const uint32_t w0 = a[0];
    uint32_t w1 = 0;
    if ((a_hi & ~(uintptr_t)3) != (a_lo & ~(uintptr_t)3)) w1 = a[1];
    return (uint64_t)w1 << 32 | w0;
}
__device__ __forceinline__ uint32_t mb_byte(uint64_t w, uintptr_t a_lo, uint32_t k) // byte a_lo + k of mb_load(a_lo, ..)
{
    return (uint32_t)(w >> (8u * ((uint32_t)(a_lo & 3u) + k))) & 255u;
}

// A thread's walk over the CIGAR of its read.
struct MbWalk {
    uint32_t k, nc;      // next operation, their number (k == nc: the walk is over, or the read does not count)
    uint32_t L, N;
    uint32_t qoff, soff, coff, info; // info: read group | mate << 8 | reverse << 9
    uint64_t j;          // stored base index
    int64_t g;           // genome position
    uint64_t len;        // the contig's length
    uintptr_t ref;       // its bytes
    // the run found last
    uint32_t ia, ib;
    uintptr_t ga;        // address of the genome byte of stored position 0 (ref + posv: may lie in front of ref; only ga + p, ia <= p < ib, is used)
};

__device__ __forceinline__ void mb_fetch(MbWalk& w, const DevBatch& b, const DevRefs& refs, uint64_t i, uint32_t end, uint32_t N, uint32_t n_lanes)
{
    w.k = w.nc = 0;
    if (i >= end) return;
    const uint32_t r = b.order ? b.order[i] : (uint32_t)i;
    if (r >= b.n_reads) return;
    const uint32_t f = b.flag[r], L = b.l_seq[r], g = b.lane[r], nc = b.n_cigar[r];
    const int32_t rid = b.rid[r];
    if ((f & 0x900u) || !(f & 0xC0u) || (f & BQC_FLAG_NO_QUAL) || (f & 0x4u) || !L || g >= n_lanes || !nc || rid < 0 || (uint32_t)rid >= refs.n_refs) return;
    const uint8_t* ref = refs.ref[rid];
    if (!ref) return;
    w.ref = (uintptr_t)ref;
    w.len = refs.len[rid];
    w.L = L; w.N = N;
    w.qoff = b.qual_off[r]; w.soff = b.seq_off[r]; w.coff = b.cigar_off[r];
    w.info = g | ((f & 0x40u) ? 0u : 1u << 8) | ((f >> 4) & 1u) << 9;
    w.j = 0;
    w.g = b.pos[r];
    w.nc = nc;
}

// the next run of the walk (false: none left)
__device__ __forceinline__ bool mb_next(MbWalk& w, const uint32_t* __restrict__ cigar)
{
    while (w.k < w.nc && w.j < w.L) { // (behind the read's last base nothing counts)
        const uint32_t wd = cigar[w.coff + w.k];
        ++w.k;
        const uint32_t op = wd & 15u;
        const uint64_t n = wd >> 4;
        if (op == 0u || op == 7u || op == 8u) {
            const int64_t posv = w.g - (int64_t)w.j;
            uint64_t lo = w.j, hi = min(w.j + n, (uint64_t)w.L);
            if (posv < 0) lo = max(lo, (uint64_t)(-posv));                       // 0 <= posv + p
            const int64_t top = (int64_t)w.len - posv;                          // posv + p < len
            hi = top <= 0 ? 0ull : min(hi, (uint64_t)top);
            if (w.info >> 9 & 1u) { if (w.L > w.N) lo = max(lo, (uint64_t)(w.L - w.N)); } // cycle L - 1 - p < N
            else hi = min(hi, (uint64_t)w.N);                                    // cycle p < N
            w.j += n;
            w.g += (int64_t)n;
            if (lo < hi) {
                w.ia = (uint32_t)lo; w.ib = (uint32_t)hi;
                w.ga = w.ref + (uintptr_t)posv;
                return true;
            }
        }
        else if (op == 1u || op == 4u) w.j += n;
        else if (op == 2u || op == 3u) w.g += (int64_t)n;
    }
    w.k = w.nc;
    return false;
}
