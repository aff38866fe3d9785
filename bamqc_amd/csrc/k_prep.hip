// k_prep.hip — the per-read pre-pass and the work decomposition of a batch, on the device.
//
// What the reference does record by record before its counters see a read is done here for a whole batch:
//   k_prep_sizes                 sums of ceil(L/2), L, n_cigar per block of 1024 reads, in two levels: inside groups of PR_GROUP blocks, and
//                                per group (prep.h); k_prep_reads adds the groups before its own — the payload offsets of every read
//                                without a serial scan between the two launches
//   k_prep_reads                 lane per read: quality-missing flag, checkFlagsAndQuality (TripletCounting.hpp:136-168)
//                                incl. the forward-only FASTA scan (:254-259) inside a block, the covered interval(s) of
//                                OverallNumbers::coverage (OverallNumbers.hpp:112-131) from the host's anchor (win, pos), the triplet
//                                segments of multi-operation CIGARs (TripletCounting.hpp:203-232), and the checks whose failure ends
//                                the reference's run (bamqualcheck.cpp:340,385-389)
//   k_build_count / _plan / _scatter   chunk tables and the entry order (`perm`) of k_short / k_reads / k_long: reads are ranked by
//                                mate slot inside super-windows of BQC_SW_READS stream positions, so that a read group of k_short holds
//                                first-mate and second-mate reads of one short stretch of the stream (shared 128-byte lines) while
//                                every lane of k_short only ever sees one mate.
// Only the O(1)-per-read coverage anchor recurrence (OverallNumbers.hpp:84-110) stays on the host (bqc_pipeline.cpp).
#include <algorithm>
#include <vector>
#include "kernels_common.h"
#include "prep.h"

#define PR_THREADS 256
#define PR_PER_THREAD 4
#define PR_BLOCK (PR_THREADS * PR_PER_THREAD) // reads per workgroup of the per-read kernels

// ---------------------------------------------------------------------------------------------------
// scans over the 256 threads of a workgroup (4 waves): DPP inside a wave, four LDS words across
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_scan_incl_max(uint32_t v) // unsigned, identity 0
{
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false));
    return v;
}
// exclusive sum over the workgroup's threads in thread order; *total = sum over all threads.  `sh`: 2 * waves words of LDS.
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* sh, uint32_t* total)
{
    const uint32_t inc = wave_scan_incl(v), w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    block_sync();
    if (lane_id() == WAVE - 1) sh[w] = inc;
    block_sync();
    uint32_t base = 0, tot = 0;
    for (uint32_t k = 0; k < nw; ++k) { const uint32_t x = sh[k]; if (k < w) base += x; tot += x; }
    *total = tot;
    return base + inc - v;
}
// exclusive sums of N values over the workgroup's threads in thread order (in place); tot: the sums over all threads.  `sh`: N * waves words.
// NW: the workgroup's waves where the kernel knows them (the loops over them unroll), 0: taken from blockDim.  between(): run by every
// thread between the two barriers — it sees what the workgroup wrote to LDS before the scan, and what it writes the workgroup sees behind it
struct NothingBetween { __device__ __forceinline__ void operator()() const {} };
template <int N, int NW = 0, class Between = NothingBetween>
__device__ __forceinline__ void block_scan_excl_n(uint32_t v[N], uint32_t* sh, uint32_t tot[N], Between between = Between())
{
    const uint32_t w = threadIdx.x >> 6, nw = NW ? NW : blockDim.x >> 6;
    uint32_t inc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) inc[k] = wave_scan_incl(v[k]);
    block_sync();
    if (lane_id() == WAVE - 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) sh[N * w + k] = inc[k];
    }
    between();
    block_sync();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        uint32_t base = 0, t = 0;
        for (uint32_t q = 0; q < nw; ++q) { const uint32_t x = sh[N * q + k]; if (q < w) base += x; t += x; }
        tot[k] = t;
        v[k] = base + inc[k] - v[k];
    }
}
template <int NW = 0>
__device__ __forceinline__ uint32_t block_scan_excl_max(uint32_t v, uint32_t* sh, uint32_t* total)
{
    const uint32_t inc = wave_scan_incl_max(v), w = threadIdx.x >> 6, nw = NW ? NW : blockDim.x >> 6;
    block_sync();
    if (lane_id() == WAVE - 1) sh[w] = inc;
    block_sync();
    uint32_t base = 0, tot = 0;
    for (uint32_t k = 0; k < nw; ++k) { const uint32_t x = sh[k]; if (k < w) base = max(base, x); tot = max(tot, x); }
    *total = tot;
    const uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x138 /* wave_shr:1 */, 0xF, 0xF, true); // inclusive value of the lane before
    return max(base, prev);
}
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) // a value every lane holds, into scalar registers
{
    return (unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)v) | (unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32;
}
__device__ __forceinline__ void err_key(ErrRec* e, uint32_t read, uint32_t order)
{
    atomicMin(&e->first_key, ((unsigned long long)read << 3) | order);
}

// ---------------------------------------------------------------------------------------------------
// payload sizes -> offsets
// ---------------------------------------------------------------------------------------------------
// One workgroup per group of PR_GROUP blocks, a wave per block (16 waves, PR_GROUP / 16 blocks each): lane l of the wave owns the reads
// 256 j + 4 l .. + 3 of the block, j = 0 .. 3 — the loads of k_prep_reads.  Every load of a wave is requested before the first sum.
#define PS_THREADS 1024
#define PS_PER (PR_GROUP / (PS_THREADS / 64))
__global__ __launch_bounds__(PS_THREADS) void k_prep_sizes(PrepArgs a)
{
    __shared__ unsigned long long sh[3 * PR_GROUP];
    if (blockIdx.x == 0 && threadIdx.x == 0) { // first kernel of the batch: its records start empty; a replayed batch starts from its own cursor
        a.err->first_key = BQC_ERRKEY_NONE; a.err->flags = 0; a.err->aux0 = a.err->aux1 = 0;
        a.desc->n_cov_extra = 0;
        if (a.pend_extra_n) *a.pend_extra_n = 0;
        if (a.replay) *a.cursor = *a.cursor_save; else *a.cursor_save = *a.cursor;
    }
    for (uint32_t k = blockIdx.x * PS_THREADS + threadIdx.x; k < a.n_sw; k += gridDim.x * PS_THREADS) a.sw_counts[k] = SwCounts{0, 0, 0, 0};
    const uint32_t nblk = (a.n + PR_BLOCK - 1) / PR_BLOCK, bg0 = blockIdx.x * PR_GROUP, nb = min((uint32_t)PR_GROUP, nblk - bg0);
    const uint32_t w = threadIdx.x >> 6, l = lane_id();
    uint4 vl[PS_PER][4];
    uint2 vc[PS_PER][4];
#pragma unroll
    for (int q = 0; q < PS_PER; ++q) {
        const uint32_t bl = w + (PS_THREADS / 64) * q;
        const unsigned long long i0 = (unsigned long long)(bg0 + bl) * PR_BLOCK;
        const bool whole = bl < nb && i0 + PR_BLOCK <= a.n;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            vl[q][j] = make_uint4(0, 0, 0, 0); vc[q][j] = make_uint2(0, 0);
            if (whole) { const uint32_t i = (uint32_t)i0 + 256u * j + 4u * l; vl[q][j] = *(const uint4*)(a.l_seq + i); vc[q][j] = *(const uint2*)(a.n_cigar + i); }
        }
    }
#pragma unroll
    for (int q = 0; q < PS_PER; ++q) {
        const uint32_t bl = w + (PS_THREADS / 64) * q;
        const unsigned long long i0 = (unsigned long long)(bg0 + bl) * PR_BLOCK;
        unsigned long long s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint4 v = vl[q][j];
            s1 += (unsigned long long)((v.x + 1) / 2) + (v.y + 1) / 2 + (v.z + 1) / 2 + (v.w + 1) / 2;
            s2 += (unsigned long long)v.x + v.y + v.z + v.w;
            s3 += (vc[q][j].x & 0xFFFFu) + (vc[q][j].x >> 16) + (vc[q][j].y & 0xFFFFu) + (vc[q][j].y >> 16);
        }
        if (bl < nb && i0 + PR_BLOCK > a.n) // the batch's last block
            for (unsigned long long i = i0 + l; i < a.n; i += WAVE) { const uint32_t L = a.l_seq[i]; s1 += (L + 1) / 2; s2 += L; s3 += a.n_cigar[i]; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); s3 += __shfl_xor(s3, o); }
        if (l == 0) { sh[3 * bl] = s1; sh[3 * bl + 1] = s2; sh[3 * bl + 2] = s3; } // (a block past the batch's end: 0)
    }
    block_sync();
    if (threadIdx.x < 3 * PR_GROUP) {
        const uint32_t bl = threadIdx.x / 3, k = threadIdx.x % 3;
        unsigned long long t = 0;
        for (uint32_t j = 0; j < bl; ++j) t += sh[3 * j + k];
        if (bl < nb) a.blk_sizes[3ull * (bg0 + bl) + k] = t;
        if (bl == PR_GROUP - 1) a.grp_sizes[3ull * blockIdx.x + k] = t + sh[3 * bl + k];
    }
}

// ---------------------------------------------------------------------------------------------------
// per read
// ---------------------------------------------------------------------------------------------------
// A read's CIGAR as the deferred path sees it: the first four words in registers, requested together, the rest from memory.
struct CigarView {
    uint32_t w[4];
    const uint32_t* cg;
    __device__ __forceinline__ uint32_t at(uint32_t k) const
    {
        if (k < 4u) return k == 0u ? w[0] : k == 1u ? w[1] : k == 2u ? w[2] : w[3];
        return cg[k];
    }
};

// One read's share of the pre-pass: everything but the payload offsets and the cross-read part of the FASTA scan.  A read whose CIGAR
// needs no walk — at most one operation, and not set aside by a shard — is done by prep_simple from CIGAR word 0, in the unrolled
// body of k_prep_reads; every other read by prep_walk, of which the kernel holds ONE copy, called in a loop over those reads.
// Round 8 carried the walks, a four-word CigarView and 64-bit interval arithmetic in each of the four unrolled copies: 128 VGPRs
// for a path that 5 % of a short-read batch's reads take.
struct ReadIn { uint32_t L, nc, flag, lane, mapq; int32_t as; CovEntry ce; };
struct ReadOut { uint32_t flag, cls, eo; CovEntry ce; }; // (its FASTA position + 1 is tgt1_in where flag has BQC_FLAG_TRIPLET)
#define PR_EO_NONE 7u // eo: the lowest order of the error keys the read raises (the lowest wins in ErrRec::first_key), PR_EO_NONE: none

// The columns of a thread's four reads as they arrive: a read's fields are taken out where it is looked at, not before.
struct Quad {
    uint32_t L[4], nc[2], flag[2], lane, mapq; // (n_cigar and flag: 16 bits a read, lane and mapq: 8)
    int32_t rid[4], as[4];
    uint32_t cov[8]; // CovEntry {win, off_len} a read
    __device__ __forceinline__ uint32_t ncig(int j) const { return (nc[j >> 1] >> (16 * (j & 1))) & 0xFFFFu; }
    __device__ __forceinline__ ReadIn read(int j) const
    {
        return ReadIn{L[j], ncig(j), (flag[j >> 1] >> (16 * (j & 1))) & 0xFFFFu, (lane >> (8 * j)) & 0xFFu, (mapq >> (8 * j)) & 0xFFu, as[j], CovEntry{cov[2 * j], cov[2 * j + 1]}};
    }
};

// What both paths do before the coverage: the checks of the read's length and read group, and — primary records only
// (bamqualcheck.cpp:318-327) — checkFlagsAndQuality (TripletCounting.hpp:136-168; `clipped()`: the CIGAR holds soft- or hard-clipped
// bases, asked last and only of a read that is eligible otherwise), the forward-only FASTA scan's own-read part (:254-259) and the
// mate check.  Returns the read's flag word with BQC_FLAG_TRIPLET decided; *eo: the lowest order of the error keys it raises — the
// thread sends ONE key, its lowest, where each check used to branch around an atomic of its own.
template <class Clipped>
__device__ __forceinline__ uint32_t read_checks(const PrepArgs& a, const ReadIn& in, uint32_t tgt1_in /* the contig's FASTA record + 1; 0: none, or not loaded */, Clipped clipped, uint32_t* eo)
{
    uint32_t flag = in.flag & (0x0FFFu | BQC_FLAG_MATE_MAIN | BQC_FLAG_NO_QUAL);
    uint32_t o = in.L > a.max_read_len ? 1u : in.lane >= a.n_lanes ? 2u : PR_EO_NONE;
    // (BQC_FLAG_NO_QUAL — quality block starting with 0xFF, SURVEY U1 — is a fact of the record's decoding and arrives with the
    // flag column: probing qual[qo] here cost one 128-byte line per read, more than every other byte this kernel reads)
    // Written as conditions, not as nested branches: the compiler then selects, where it used to jump around every step.
    const bool primary = !(flag & 0x900u);
    const bool counted = primary && !(flag & 0x600u);                                  // neither duplicate nor QC fail: tripletCounting, :338-342
    const bool mapped_pair = (flag & 0x10Fu) == 0x3u && in.mapq >= 60;                 // paired, proper, neither mate unmapped, not secondary
    const bool as_bad = in.as == BQC_AS_ABSENT || in.as < 0;                           // (fatal for a read that got this far)
    bool eligible = counted && mapped_pair && !as_bad && in.as >= 50;
    if (eligible) eligible = !clipped();
    if (counted && mapped_pair && as_bad) o = min(o, 4u);
    if (eligible && !tgt1_in) o = min(o, 5u);                                          // Genome: forward-only FASTA scan, no record for the contig
    if (eligible && tgt1_in) flag |= BQC_FLAG_TRIPLET;
    if (primary && !(flag & 0xC0u)) o = min(o, 6u);
    *eo = o;
    return flag;
}
__device__ __forceinline__ uint32_t mate_class(const PrepArgs& a, uint32_t flag, uint32_t L) // mate slot of a fast read (first mate / everything else) or 2 = generic path
{
    return !a.no_fast && L <= BQC_FAST_MAXLEN ? ((flag & 0x40u) ? 0u : 1u) : 2u;
}

// nc <= 1, ce.win != BQC_COV_PENDING: `w0` is the CIGAR's one word (0: none).  No segment, no second interval.
__device__ __forceinline__ ReadOut prep_simple(const PrepArgs& a, const ReadIn& in, uint32_t w0, uint32_t tgt1_in)
{
    const uint32_t op = w0 & 15u, nn = w0 >> 4;
    ReadOut o;
    o.flag = read_checks(a, in, tgt1_in, [&] { return (op == 4u || op == 5u) && nn > 0; }, &o.eo);
    o.ce = CovEntry{in.ce.win, 0};
    if (in.ce.win != BQC_COV_NONE) { // OverallNumbers.hpp:112-131 for one operation: [pos, pos + nn) cut at 2 * BQC_VSIZE
        o.flag |= BQC_FLAG_COV;
        const uint32_t pos = in.ce.off_len;
        if ((op == 0u || op == 2u) && pos < 2u * BQC_VSIZE) { // (pos + nn < 2^32 here)
            const uint32_t hi = min(pos + nn, 2u * BQC_VSIZE);
            if (pos < hi) o.ce.off_len = pos | ((hi - pos) << 16);
        }
    }
    o.cls = mate_class(a, o.flag, in.L) << 8;
    return o;
}

// Any read: several operations, a set-aside read of a shard, or a read whose CIGAR is not looked at (offsets_ok false: the batch fails
// with the block's check in k_prep_reads).  Reloads the read's columns — they have just been read by this workgroup — and its CIGAR.
__device__ __forceinline__ ReadOut prep_walk(const PrepArgs& a, uint32_t i, uint32_t nc_in, uint32_t co, bool offsets_ok, uint32_t tgt1_in)
{
    const ReadIn in{a.l_seq[i], offsets_ok ? nc_in : 0u, a.flag_in[i], a.lane[i], a.mapq[i], a.as_[i], a.cov_in[i]};
    const int32_t bam_pos = a.pos[i];
    const uint32_t L = in.L, lane = in.lane, nc = in.nc;
    CigarView cv;
    cv.cg = a.cigar + co;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) cv.w[k] = k < nc ? cv.cg[k] : 0u;
    ReadOut o;
    uint32_t flag = read_checks(a, in, tgt1_in, [&] {
        uint32_t clipped = 0;
        for (uint32_t k = 0; k < nc; ++k) {
            const uint32_t wd = cv.at(k), op = wd & 15u;
            if (op == 4u || op == 5u) clipped += wd >> 4;
        }
        return clipped > 0;
    }, &o.eo);
    const uint32_t cl = mate_class(a, flag, L);
    uint32_t nseg = 0;
    CovEntry ce = in.ce;
    // The read's covered interval(s) relative to its first live window (OverallNumbers.hpp:112-131): `c` runs over the
    // seq-oriented CIGAR (reversed for reverse reads, bamqualcheck.cpp:349) and advances on S, M and D; M and D add
    // coverage.  DEFINED: increments at window offset >= 2000 are dropped.  One interval unless a clip sits between
    // two match operations.  The host decided WHETHER the read enters coverage() and where its window starts.
    if (ce.win != BQC_COV_NONE) {
        flag |= BQC_FLAG_COV;
        const bool rc = flag & 0x10u;
        const bool pending = ce.win == BQC_COV_PENDING; // shard mode: the window comes later (bqc_shard_resolve): runs relative to beginPos
        const uint32_t pend_idx = ce.off_len;
        const int64_t pos = pending ? 0 : (int64_t)ce.off_len;
        uint32_t cc = 0; // `int c` in the reference; wraps identically
        int64_t run_a = -1, run_z = -1;
        bool first = true;
        ce.off_len = 0;
        auto emit = [&](int64_t lo, int64_t hi) {
            if (pending) { // (pos <= 2000 later: a run that starts 2000 or more behind beginPos can never count)
                if (lo < 0 || lo >= 2 * BQC_VSIZE || lo >= hi) return;
                const uint32_t len = (uint32_t)(hi - lo < 2 * BQC_VSIZE ? hi - lo : 2 * BQC_VSIZE);
                if (first) { a.pend[pend_idx] = PendRun{(uint32_t)lo, len}; first = false; return; }
                const uint32_t k = atomicAdd(a.pend_extra_n, 1u);
                if (k < a.pend_extra_cap) a.pend_extra[k] = PendExtra{pend_idx, (uint32_t)lo, len, 0};
                else atomicOr(&a.err->flags, BQC_DEVERR_INTERNAL);
                return;
            }
            hi = hi < 2 * BQC_VSIZE ? hi : 2 * BQC_VSIZE;
            if (lo < 0 || lo >= hi) return;
            const uint32_t v = (uint32_t)lo | ((uint32_t)(hi - lo) << 16);
            if (first) { ce.off_len = v; first = false; return; }
            const uint32_t k = atomicAdd(&a.desc->n_cov_extra, 1u);
            if (k < a.cov_extra_cap) a.cov_extra[k] = CovExtra{ce.win, v, lane, 0};
            else atomicOr(&a.err->flags, BQC_DEVERR_INTERNAL); // (capacity = CIGAR words / 2 + 1: cannot happen)
        };
        if (nc == 1u) {
            const uint32_t w = cv.w[0], op = w & 15u, nn = w >> 4;
            if (op == 0u || op == 2u) emit(pos, pos + nn);
        } else {
            for (uint32_t k = 0; k < nc; ++k) {
                const uint32_t w = cv.at(rc ? nc - 1 - k : k), op = w & 15u, nn = w >> 4;
                if (op == 4u) cc += nn;
                if (op == 0u || op == 2u) {
                    const int64_t lo = pos + (int64_t)cc, hi = lo + nn;
                    if (run_z == lo) run_z = hi;
                    else { if (run_a >= 0) emit(run_a, run_z); run_a = lo; run_z = hi; }
                    cc += nn;
                }
            }
            if (run_a >= 0) emit(run_a, run_z);
        }
        if (pending) { if (first) a.pend[pend_idx] = PendRun{0, 0}; ce = CovEntry{BQC_COV_NONE, 0}; }
    } else ce.off_len = 0;
    // k_short evaluates triplets with chromPos = pos + i inside the first CIGAR operation (assumed match-like,
    // TripletCounting.hpp:203); every further match-like operation becomes a segment entry with its own offset
    if (cl != 2u && (flag & BQC_FLAG_TRIPLET) && nc > 1 && L >= 3) {
        const uint32_t n0 = cv.w[0] >> 4;
        if (n0 != 0) { // (n0 == 0: every position counts as inside the first operation, no walk)
            uint64_t rp = n0;
            int64_t cpos = (int64_t)bam_pos + n0;
            for (uint32_t k2 = 1; k2 < nc && rp < L; ++k2) {
                const uint32_t wk = cv.at(k2), op = wk & 15u, nn = wk >> 4;
                if (op == 2u || op == 3u || op == 5u || op == 6u) cpos += nn;   // D N H P
                else if (op == 4u || op == 1u) rp += nn;                          // S I
                else {                                                            // M = X (and unknown)
                    const uint64_t ia = rp > 1 ? rp : 1, ib = rp + nn < (uint64_t)L - 1 ? rp + nn : (uint64_t)L - 1;
                    const int64_t posv = cpos - (int64_t)rp;
                    if (ia < ib && posv > INT32_MIN / 2 && posv < INT32_MAX / 2) {
                        a.segs[co + nseg] = TripSeg{i, (int32_t)posv, (uint32_t)ia | ((uint32_t)ib << 8), 0};
                        ++nseg;
                    }
                    rp += nn; cpos += nn;
                }
            }
        }
    }
    o.flag = flag;
    o.ce = ce;
    o.cls = (cl << 8) | nseg;
    return o;
}
__device__ __forceinline__ uint32_t pick4(const uint32_t v[4], uint32_t j) { return j == 0u ? v[0] : j == 1u ? v[1] : j == 2u ? v[2] : v[3]; }

// Thread t of a workgroup owns the four consecutive reads b0 + 4t .. + 3: their columns are 8- / 16-byte loads, the payload
// offsets are a serial prefix inside the thread plus ONE three-wide workgroup scan, and so is the forward-only FASTA scan.
#ifndef PR_WAVES_PER_EU
#define PR_WAVES_PER_EU 5
#endif
__global__ __launch_bounds__(PR_THREADS) __attribute__((amdgpu_waves_per_eu(PR_WAVES_PER_EU, PR_WAVES_PER_EU))) void k_prep_reads(PrepArgs a, DevRefs refs)
{
    __shared__ uint32_t sh[3 * (PR_THREADS / 64)];
    __shared__ uint32_t red[8];
    __shared__ unsigned long long gsum[3 * (PR_THREADS / 64) + 6], gtot[3];
    const uint32_t i0 = blockIdx.x * PR_BLOCK + 4u * threadIdx.x;
    if (threadIdx.x < 8) red[threadIdx.x] = threadIdx.x == 0 ? 0xFFFFFFFFu : 0u;
    // The block's bases: the totals of the groups before this block's (thread t: groups t, t + 256, ..) and the sums inside the group up
    // to this block, without and with it (threads 0 .. 5, a word each).  Requested in front of the columns — loads return in the order of their requests —
    // and summed while the columns are in flight: no round trip in front of them, and none behind.
    const uint32_t grp = blockIdx.x / PR_GROUP, nblk = gridDim.x;
    unsigned long long grp_before[3] = {0, 0, 0}, grp_more[3] = {0, 0, 0}, in_grp = 0;
    for (uint32_t g = threadIdx.x + 2 * PR_THREADS; g < grp; g += PR_THREADS) { // (more than 512 groups, batches of more than 16 M reads: waited for here)
        const unsigned long long* p = (const unsigned long long*)((const char*)a.grp_sizes + 24u * g); // (a 32-bit offset from a scalar base)
        for (int k = 0; k < 3; ++k) grp_before[k] += p[k];
    }
    if (threadIdx.x < grp) {
        const unsigned long long* p = (const unsigned long long*)((const char*)a.grp_sizes + 24u * threadIdx.x);
        for (int k = 0; k < 3; ++k) grp_before[k] += p[k];
    }
    if (threadIdx.x + PR_THREADS < grp) {
        const unsigned long long* p = (const unsigned long long*)((const char*)a.grp_sizes + 24u * (threadIdx.x + PR_THREADS));
        for (int k = 0; k < 3; ++k) grp_more[k] = p[k];
    }
    if (threadIdx.x < 6) { // (a word per lane: loads the wave does not wait for here, as it would for scalar ones)
        const bool grp_last = (blockIdx.x + 1) % PR_GROUP == 0 || blockIdx.x + 1 == nblk;
        const unsigned long long* incl_p = grp_last ? a.grp_sizes + 3ull * grp : a.blk_sizes + 3ull * (blockIdx.x + 1);
        in_grp = threadIdx.x < 3 ? a.blk_sizes[3ull * blockIdx.x + threadIdx.x] : incl_p[threadIdx.x - 3];
    }
    auto sum_groups = [&] { // over the workgroup, into LDS: read behind the barriers of the scan below.  A wave's LDS operations run in
        // their order: its lane 0 clears the wave's three words, then the lanes that hold a group add to them
        unsigned long long* mine = gsum + 3 * (threadIdx.x >> 6);
        if (lane_id() == 0) for (int k = 0; k < 3; ++k) mine[k] = 0;
        if (threadIdx.x < grp) for (int k = 0; k < 3; ++k) atomicAdd(mine + k, grp_before[k] + grp_more[k]);
        if (threadIdx.x < 6) gsum[3 * (PR_THREADS / 64) + threadIdx.x] = in_grp;
    };
    Quad q;
    const uint32_t nlive = i0 >= a.n ? 0u : min(4u, a.n - i0);
    if ((unsigned long long)(blockIdx.x + 1) * PR_BLOCK <= a.n) { // (every block but a batch's last: the same for all its threads, so that they can sum together inside)
        const uint4 vl = *(const uint4*)(a.l_seq + i0);
        const uint2 vc = *(const uint2*)(a.n_cigar + i0), vf = *(const uint2*)(a.flag_in + i0);
        const uint32_t vlane = *(const uint32_t*)(a.lane + i0), vmq = *(const uint32_t*)(a.mapq + i0);
        const int4 vr = *(const int4*)(a.rid + i0), va = *(const int4*)(a.as_ + i0);
        const uint4 c01 = *(const uint4*)(a.cov_in + i0), c23 = *(const uint4*)(a.cov_in + i0 + 2);
        // (the sums are taken HERE, while the columns are in flight: without this the compiler adds the two loaded halves, and waits
        // for them, in front of the column loads)
        asm volatile("" : "+v"(grp_before[0]), "+v"(grp_before[1]), "+v"(grp_before[2]));
        sum_groups();
        q = Quad{{vl.x, vl.y, vl.z, vl.w}, {vc.x, vc.y}, {vf.x, vf.y}, vlane, vmq, {vr.x, vr.y, vr.z, vr.w}, {va.x, va.y, va.z, va.w},
                 {c01.x, c01.y, c01.z, c01.w, c23.x, c23.y, c23.z, c23.w}};
    } else {
        sum_groups();
        q = Quad{{0, 0, 0, 0}, {0, 0}, {0x09000900u, 0x09000900u}, 0, 0, {-1, -1, -1, -1}, {0, 0, 0, 0}, {BQC_COV_NONE, 0, BQC_COV_NONE, 0, BQC_COV_NONE, 0, BQC_COV_NONE, 0}};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((uint32_t)j < nlive) {
                const uint32_t i = i0 + j, h = 16 * (j & 1);
                const CovEntry ce = a.cov_in[i];
                q.L[j] = a.l_seq[i]; q.rid[j] = a.rid[i]; q.as[j] = a.as_[i]; q.cov[2 * j] = ce.win; q.cov[2 * j + 1] = ce.off_len;
                q.nc[j >> 1] |= (uint32_t)a.n_cigar[i] << h; q.flag[j >> 1] = (q.flag[j >> 1] & ~(0xFFFFu << h)) | ((uint32_t)a.flag_in[i] << h);
                q.lane |= (uint32_t)a.lane[i] << (8 * j); q.mapq |= (uint32_t)a.mapq[i] << (8 * j);
            }
    }
    // payload offsets: prefix inside the thread, then across the workgroup
    uint32_t ls[4], lq[4], lc[4], x[3] = {0, 0, 0}, tot[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) { ls[j] = x[0]; lq[j] = x[1]; lc[j] = x[2]; x[0] += (q.L[j] + 1) / 2; x[1] += q.L[j]; x[2] += q.ncig(j); }
    block_scan_excl_n<3, PR_THREADS / 64>(x, sh, tot, [&] { // (the waves' group sums, added by three threads: nine words for every thread to read, not 18)
        if (threadIdx.x < 3) {
            unsigned long long t = 0;
            for (uint32_t w = 0; w < PR_THREADS / 64; ++w) t += gsum[3 * w + threadIdx.x];
            gtot[threadIdx.x] = t;
        }
    });
    unsigned long long excl[3], incl[3];
    for (int k = 0; k < 3; ++k) { // (behind the scan's barriers; the same in every lane: scalar registers)
        grp_before[k] = uniform64(gtot[k]); excl[k] = uniform64(gsum[3 * (PR_THREADS / 64) + k]); incl[k] = uniform64(gsum[3 * (PR_THREADS / 64) + 3 + k]);
    }
    unsigned long long base[3];
    const bool over = prep_block_bases(grp_before, excl, incl, base); // (the same in every lane)
    if (over && threadIdx.x == 0) err_key(a.err, blockIdx.x * PR_BLOCK, 3);
    const uint32_t bs = (uint32_t)base[0] + x[0], bq = (uint32_t)base[1] + x[1], bc = (uint32_t)base[2] + x[2];
    uint32_t bad = 0; // reads whose payload ends leave 32 bits: the block's end does, in some quantity (the batch fails)
    if (over) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long so = base[0] + x[0] + ls[j], qo = base[1] + x[1] + lq[j], co = base[2] + x[2] + lc[j];
            if (so + (q.L[j] + 1) / 2 > 0xFFFFFFFFull || qo + q.L[j] > 0xFFFFFFFFull || co + q.ncig(j) > 0xFFFFFFFFull) bad |= 1u << j;
        }
        bad &= (1u << nlive) - 1u;
    }
    // the offsets leave first: nothing below changes them
    const uint32_t cos[4] = {bc + lc[0], bc + lc[1], bc + lc[2], bc + lc[3]};
    if (nlive == 4u) {
        *(uint4*)(a.seq_off + i0) = make_uint4(bs + ls[0], bs + ls[1], bs + ls[2], bs + ls[3]);
        *(uint4*)(a.qual_off + i0) = make_uint4(bq + lq[0], bq + lq[1], bq + lq[2], bq + lq[3]);
        *(uint4*)(a.cigar_off + i0) = make_uint4(cos[0], cos[1], cos[2], cos[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) // (constant indices: a thread's arrays stay in registers)
            if ((uint32_t)j < nlive) { a.seq_off[i0 + j] = bs + ls[j]; a.qual_off[i0 + j] = bq + lq[j]; a.cigar_off[i0 + j] = cos[j]; }
    }
    // what the four reads need from memory besides their columns, all of it requested before the first read is looked at: CIGAR word 0
    // and the contig's entries of the reference tables.  `walk`: the reads that go through prep_walk
    uint32_t w0[4], tgt1[4], walk = 0, maxfast = 0, maxlong = 0;
    const uint8_t* ref_ptr[4]; // (taken as values and looked at behind the last request: `rid_ok && refs.ref[rid] != nullptr` made the wave wait for each one in turn)
    int32_t target[4];         // the contig's FASTA record, -1: none
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool live = (uint32_t)j < nlive, ok = !((bad >> j) & 1u);
        const uint32_t nc = q.ncig(j), L = q.L[j];
        if (live && (!ok || nc > 1u || q.cov[2 * j] == BQC_COV_PENDING)) walk |= 1u << j;
        w0[j] = live && ok && nc ? a.cigar[cos[j]] : 0u;
        const int32_t rid = q.rid[j];
        const bool rid_ok = live && rid >= 0 && (uint32_t)rid < refs.n_refs;
        ref_ptr[j] = rid_ok ? refs.ref[rid] : nullptr;
        target[j] = rid_ok ? rid : -1;
        const bool fast = !a.no_fast && L <= BQC_FAST_MAXLEN; // (mate_class: the CIGAR has no say)
        maxfast = max(maxfast, live && fast ? L : 0u); maxlong = max(maxlong, live && !fast ? L : 0u);
    }
    if (a.fasta_index) { // (a branch of its own, the same for every thread: inside the loop above each of these loads was waited for where it stood)
#pragma unroll
        for (int j = 0; j < 4; ++j) if (target[j] >= 0) target[j] = a.fasta_index[target[j]];
    }
    // (nothing is derived from one of these words before all are requested: the compiler would put the test right behind each load)
    asm volatile("" : "+v"(target[0]), "+v"(target[1]), "+v"(target[2]), "+v"(target[3]), "+v"(ref_ptr[0]), "+v"(ref_ptr[1]), "+v"(ref_ptr[2]), "+v"(ref_ptr[3]));
#pragma unroll
    for (int j = 0; j < 4; ++j) tgt1[j] = ref_ptr[j] != nullptr && target[j] >= 0 ? (uint32_t)target[j] + 1u : 0u;
    // the reads that need no walk, and the thread's 8- and 16-byte stores; a read of the other kind leaves them as no read at all
    uint32_t fc[4]; // flag | cls << 16: what the thread still needs of a read once it is stored
    uint32_t ekey = 0xFFFFFFFFu; // the thread's lowest error key, (read - i0) << 3 | order
    {
        ReadOut out[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            out[j] = ReadOut{0x900u, 2u << 8, PR_EO_NONE, CovEntry{BQC_COV_NONE, 0}};
            if ((uint32_t)j < nlive && !((walk >> j) & 1u)) out[j] = prep_simple(a, q.read(j), w0[j], tgt1[j]);
            fc[j] = out[j].flag | (out[j].cls << 16);
            if (out[j].eo != PR_EO_NONE) ekey = min(ekey, (uint32_t)j << 3 | out[j].eo);
        }
        if (nlive == 4u) {
            *(uint2*)(a.flag_out + i0) = make_uint2((fc[0] & 0xFFFFu) | (fc[1] << 16), (fc[2] & 0xFFFFu) | (fc[3] << 16));
            *(uint2*)(a.cls + i0) = make_uint2((fc[0] >> 16) | (fc[1] & 0xFFFF0000u), (fc[2] >> 16) | (fc[3] & 0xFFFF0000u));
            *(uint4*)(a.cov_out + i0) = make_uint4(out[0].ce.win, out[0].ce.off_len, out[1].ce.win, out[1].ce.off_len);
            *(uint4*)(a.cov_out + i0 + 2) = make_uint4(out[2].ce.win, out[2].ce.off_len, out[3].ce.win, out[3].ce.off_len);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((uint32_t)j < nlive) { a.flag_out[i0 + j] = (uint16_t)fc[j]; a.cls[i0 + j] = (uint16_t)(fc[j] >> 16); a.cov_out[i0 + j] = out[j].ce; }
        }
    }
    // the other reads, one after another through the kernel's one copy of prep_walk: each stores its own entries over the thread's
    // (a thread's stores to one address arrive in their order).  A short-read batch: one read in twenty.
#pragma nounroll
    for (uint32_t m = walk; m; m &= m - 1u) {
        const uint32_t jj = (uint32_t)__ffs((int)m) - 1u, i = i0 + jj;
        const uint32_t nc = ((jj & 2u ? q.nc[1] : q.nc[0]) >> (16u * (jj & 1u))) & 0xFFFFu;
        const ReadOut r = prep_walk(a, i, nc, pick4(cos, jj), !((bad >> jj) & 1u), pick4(tgt1, jj));
        a.flag_out[i] = (uint16_t)r.flag; a.cls[i] = (uint16_t)r.cls; a.cov_out[i] = r.ce;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) if (jj == j) fc[j] = r.flag | (r.cls << 16);
        if (r.eo != PR_EO_NONE) ekey = min(ekey, jj << 3 | r.eo);
    }
    // the four reads in their order, whichever path each took
    uint32_t tmax = 0, tmin = 0xFFFFFFFFu, cnt = 0, nseg = 0; // cnt: reads per class, 9 bits each (a wave holds 256 reads)
    bool local_bad[4] = {false, false, false, false};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!(fc[j] & BQC_FLAG_TRIPLET)) tgt1[j] = 0; // (from here on: the FASTA position + 1 of an ELIGIBLE read)
        if ((uint32_t)j >= nlive) continue;
        if (tgt1[j]) { local_bad[j] = tgt1[j] < tmax; tmax = max(tmax, tgt1[j]); tmin = min(tmin, tgt1[j]); }
        cnt += 1u << (9u * (fc[j] >> 24)); nseg += (fc[j] >> 16) & 0xFFu;
    }
    // forward-only FASTA scan: an eligible read whose position lies before an earlier eligible read's — inside the thread
    // (local_bad), inside the workgroup (here), across workgroups (k_build_plan)
    uint32_t blk_max;
    const uint32_t before = block_scan_excl_max<PR_THREADS / 64>(tmax, sh, &blk_max);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (tgt1[j] && (local_bad[j] || tgt1[j] < before)) ekey = min(ekey, (uint32_t)j << 3 | 5u);
    if (ekey != 0xFFFFFFFFu) err_key(a.err, i0 + (ekey >> 3), ekey & 7u);
    // block partials: FASTA positions (for the scan across blocks), longest fast / generic read; class counts of the super-window
    if (tmin != 0xFFFFFFFFu) atomicMin(&red[0], tmin);
    if (maxfast) atomicMax(&red[1], maxfast);
    if (maxlong) atomicMax(&red[2], maxlong);
    if (!a.order) { // stream order: the block's reads lie in one super-window
        const uint32_t c = wave_scan_incl(cnt), sg = wave_scan_incl(nseg); // (sums in the wave's last lane)
        if (lane_id() == WAVE - 1) {
            for (uint32_t k = 0; k < 3u; ++k) { const uint32_t v = (c >> (9u * k)) & 0x1FFu; if (v) atomicAdd(&red[4 + k], v); }
            if (sg) atomicAdd(&red[7], sg);
        }
    }
    block_sync();
    if (threadIdx.x == 0) {
        a.blk_tgt[2ull * blockIdx.x] = blk_max;
        a.blk_tgt[2ull * blockIdx.x + 1] = red[0];
        a.blk_maxfast[2ull * blockIdx.x] = red[1];
        a.blk_maxfast[2ull * blockIdx.x + 1] = red[2];
    }
    if (!a.order && threadIdx.x < 4 && red[4 + threadIdx.x])
        atomicAdd((uint32_t*)&a.sw_counts[blockIdx.x / (BQC_SW_READS / PR_BLOCK)] + threadIdx.x, red[4 + threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------
// chunk builder
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t read_class(const PrepArgs& a, uint32_t r, uint32_t* nseg) // 0 / 1: fast read by mate slot, 2: generic path
{
    const uint32_t v = a.cls[r];
    *nseg = v & 0xFFu;
    return v >> 8;
}

// (only for batches with several read groups: in stream order k_prep_reads has counted the classes already)
__global__ __launch_bounds__(PR_THREADS) void k_build_count(PrepArgs a)
{
    __shared__ uint32_t sh[4 * (PR_THREADS / 64)];
    const SuperWindow sw = a.sws[blockIdx.x];
    uint32_t c[4] = {0, 0, 0, 0};
    for (uint32_t p = threadIdx.x; p < sw.count; p += PR_THREADS) {
        const uint32_t r = a.order ? a.order[sw.begin + p] : sw.begin + p;
        uint32_t ns;
        const uint32_t cl = read_class(a, r, &ns);
        c[cl] += 1;
        c[3] += ns;
    }
    for (int k = 0; k < 4; ++k) c[k] = wave_sum(c[k]);
    if (lane_id() == 0) for (int k = 0; k < 4; ++k) sh[4 * (threadIdx.x >> 6) + k] = c[k];
    block_sync();
    if (threadIdx.x < 4) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < PR_THREADS / 64; ++w) t += sh[4 * w + threadIdx.x];
        ((uint32_t*)&a.sw_counts[blockIdx.x])[threadIdx.x] = t;
    }
}

// One workgroup.  (1) the forward-only FASTA scan across blocks, and the stream's cursor; (2) lanes per read of k_short;
// (3) where every super-window's entries go and the chunk tables; (4) the batch descriptor.
__global__ __launch_bounds__(1024) void k_build_plan(PrepArgs a)
{
    __shared__ uint32_t sh[2 * 16 + 8];
    __shared__ uint32_t s_fast_w, s_first_bad, s_gmin;
    const uint32_t nblk = (a.n + PR_BLOCK - 1) / PR_BLOCK;
    // ---- (1) + (2)
    {
        uint32_t carry = (uint32_t)(*a.cursor + 1); // position + 1 of the last eligible read of the stream so far (0: none)
        uint32_t mf = 0, gmin = 0xFFFFFFFFu;
        if (threadIdx.x == 0) { s_first_bad = 0xFFFFFFFFu; s_gmin = 0xFFFFFFFFu; }
        for (uint32_t b0 = 0; b0 < nblk; b0 += blockDim.x) {
            const uint32_t b = b0 + threadIdx.x;
            const uint32_t mx = b < nblk ? a.blk_tgt[2ull * b] : 0u, mn = b < nblk ? a.blk_tgt[2ull * b + 1] : 0xFFFFFFFFu;
            if (b < nblk) mf = max(mf, a.blk_maxfast[2ull * b]);
            uint32_t tot;
            const uint32_t before = max(carry, block_scan_excl_max(mx, sh, &tot));
            gmin = min(gmin, mn);
            if (mn < before) atomicMin(&s_first_bad, b); // some eligible read of block b lies before an earlier block's
            carry = max(carry, tot);
        }
        if (gmin != 0xFFFFFFFFu) atomicMin(&s_gmin, gmin);
        block_sync();
        const uint32_t bad = s_first_bad;
        if (bad != 0xFFFFFFFFu) { // find the first such read of that block (rare: the run ends with an error)
            uint32_t before = (uint32_t)(*a.cursor + 1);
            for (uint32_t b = threadIdx.x; b < bad; b += blockDim.x) before = max(before, a.blk_tgt[2ull * b]);
            uint32_t tot;
            (void)block_scan_excl_max(before, sh, &tot);
            for (uint32_t i = bad * PR_BLOCK + threadIdx.x; i < min(a.n, (bad + 1) * PR_BLOCK); i += blockDim.x)
                if (a.flag_out[i] & BQC_FLAG_TRIPLET) {
                    const int32_t rid = a.rid[i];
                    const uint32_t t1 = (uint32_t)(a.fasta_index ? a.fasta_index[rid] : rid) + 1u;
                    if (t1 < tot) err_key(a.err, i, 5);
                }
        }
        for (int o = 32; o > 0; o >>= 1) mf = max(mf, (uint32_t)__shfl_xor((int)mf, o));
        block_sync();
        if (lane_id() == 0) sh[threadIdx.x >> 6] = mf;
        block_sync();
        if (threadIdx.x == 0) {
            uint32_t m = 0;
            for (uint32_t w = 0; w < blockDim.x / 64; ++w) m = max(m, sh[w]);
            s_fast_w = max(1u, (m + 8 * BQC_FAST_NH - 1) / (8 * BQC_FAST_NH));
            *a.cursor = (int32_t)carry - 1;
            if (a.cursor[1] < 0 && s_gmin != 0xFFFFFFFFu) a.cursor[1] = (int32_t)s_gmin - 1; // first eligible read of the stream (shards check their order with it)
        }
        block_sync();
    }
    const uint32_t fast_w = s_fast_w, rpw = 64u / fast_w, h0 = (rpw + 1) / 2, h1 = rpw / 2;
    const uint32_t groups_cap = BQC_FAST_WAVES * (64u / rpw);  // groups per chunk: one tile of whole groups per wave of k_short
    const uint32_t seg_cap = groups_cap * rpw;                 // segment entries per chunk
    // ---- (3) prefix sums over the super-windows of {groups, segments, generic reads}
    uint32_t run_g = 0, run_q = 0, run_s = 0;
    for (uint32_t s0 = 0; s0 < a.n_sw; s0 += blockDim.x) {
        const uint32_t s = s0 + threadIdx.x;
        uint32_t g = 0, q = 0, sl = 0;
        if (s < a.n_sw) {
            const SwCounts c = a.sw_counts[s];
            g = max((c.n0 + h0 - 1) / h0, (c.n1 + h1 - 1) / h1);
            q = c.n_seg; sl = c.n_slow;
        }
        uint32_t tg, tq, ts;
        const uint32_t eg = run_g + block_scan_excl(g, sh, &tg), eq = run_q + block_scan_excl(q, sh, &tq), es = run_s + block_scan_excl(sl, sh, &ts);
        if (s < a.n_sw) a.sw_plan[s] = SwPlan{eg, g, eq, es}; // (relative to the batch; made absolute below)
        run_g += tg; run_q += tq; run_s += ts;
    }
    __threadfence_block();
    block_sync();
    // per stretch (one read group each, in order): [read groups | segment entries, padded to whole groups | generic reads]
    // -> absolute perm positions and chunk tables.  Thread 0 walks the stretches (at most one per read group); all threads fill.
    __shared__ uint32_t s_pb, s_cf, s_cs, s_g0, s_q0, s_s0, s_ng, s_nq, s_ns, s_lane, s_sw0, s_sw1, s_longest;
    if (threadIdx.x == 0) { s_pb = 0; s_cf = 0; s_cs = 0; }
    block_sync();
    for (uint32_t st = 0; st < a.n_stretch; ++st) {
        if (threadIdx.x == 0) {
            const Stretch S = a.stretches[st];
            const SwPlan p0 = a.sw_plan[S.sw_begin];
            const SwPlan pl = a.sw_plan[S.sw_end - 1];
            const SwCounts cl = a.sw_counts[S.sw_end - 1];
            s_g0 = p0.group_base; s_q0 = p0.seg_base; s_s0 = p0.slow_base;
            s_ng = pl.group_base + pl.n_groups - p0.group_base;
            s_nq = pl.seg_base + cl.n_seg - p0.seg_base;
            s_ns = pl.slow_base + cl.n_slow - p0.slow_base;
            s_lane = S.lane; s_sw0 = S.sw_begin; s_sw1 = S.sw_end;
        }
        block_sync();
        const uint32_t pb = s_pb, ng = s_ng, nq = s_nq, ns = s_ns, lane = s_lane;
        const uint32_t nq_pad = (nq + rpw - 1) / rpw * rpw;
        const uint32_t seg0 = pb + ng * rpw, slow0 = seg0 + nq_pad;
        for (uint32_t s = s_sw0 + threadIdx.x; s < s_sw1; s += blockDim.x) {
            SwPlan p = a.sw_plan[s];
            p.group_base = pb + (p.group_base - s_g0) * rpw;
            p.seg_base = seg0 + (p.seg_base - s_q0);
            p.slow_base = slow0 + (p.slow_base - s_s0);
            a.sw_plan[s] = p;
        }
        for (uint32_t k = nq + threadIdx.x; k < nq_pad; k += blockDim.x) a.perm[seg0 + k] = 0xFFFFFFFFu;
        const uint32_t n_rc = (ng + groups_cap - 1) / groups_cap, n_sc = (nq_pad + seg_cap - 1) / seg_cap, n_lc = (ns + BQC_CHUNK_READS - 1) / BQC_CHUNK_READS;
        const uint32_t cf = s_cf, cs = s_cs;
        for (uint32_t k = threadIdx.x; k < n_rc; k += blockDim.x) {
            const uint32_t g = min(groups_cap, ng - k * groups_cap);
            if (cf + k < a.chunks_fast_cap) a.chunks_fast[cf + k] = Chunk{pb + k * groups_cap * rpw, g * rpw, lane, g * rpw, 0, 0, 0, 0};
        }
        for (uint32_t k = threadIdx.x; k < n_sc; k += blockDim.x) {
            const uint32_t e = min(seg_cap, nq_pad - k * seg_cap);
            if (cf + n_rc + k < a.chunks_fast_cap) a.chunks_fast[cf + n_rc + k] = Chunk{seg0 + k * seg_cap, e, lane, 0, 0, 0, 0, 0};
        }
        for (uint32_t k = threadIdx.x; k < n_lc; k += blockDim.x) {
            const uint32_t e = min((uint32_t)BQC_CHUNK_READS, ns - k * BQC_CHUNK_READS);
            if (cs + k < a.chunks_slow_cap) a.chunks_slow[cs + k] = Chunk{slow0 + k * BQC_CHUNK_READS, e, lane, 0, 0, 0, 0, 0};
        }
        block_sync();
        if (threadIdx.x == 0) { s_pb = slow0 + ns; s_cf = cf + n_rc + n_sc; s_cs = cs + n_lc; }
        block_sync();
    }
    // ---- (4) descriptor; the longest generic read (the cycle tiles k_long needs)
    uint32_t longest = 0;
    for (uint32_t b = threadIdx.x; b < nblk; b += blockDim.x) longest = max(longest, a.blk_maxfast[2ull * b + 1]);
    for (int o = 32; o > 0; o >>= 1) longest = max(longest, (uint32_t)__shfl_xor((int)longest, o));
    if (threadIdx.x == 0) s_longest = 0;
    block_sync();
    if (lane_id() == 0) atomicMax(&s_longest, longest);
    block_sync();
    if (threadIdx.x == 0) {
        if (s_pb > a.perm_cap || s_cf > a.chunks_fast_cap || s_cs > a.chunks_slow_cap) atomicOr(&a.err->flags, BQC_DEVERR_INTERNAL);
        // A read that ends the reference's run (first_key) poisons the context on the host; until the host gets to know, the
        // hot kernels must not touch such a batch (a lane out of range would index outside the state vector).
        const bool fatal = a.err->first_key != BQC_ERRKEY_NONE || (a.err->flags & BQC_DEVERR_INTERNAL);
        a.desc->fatal = fatal ? 1u : 0u;
        a.desc->n_chunks_fast = fatal ? 0u : min(s_cf, a.chunks_fast_cap);
        a.desc->n_chunks_slow = fatal ? 0u : min(s_cs, a.chunks_slow_cap);
        a.desc->fast_w = fast_w;
        a.desc->n_perm = s_pb;
        a.desc->long_max_len = s_longest;
        if (a.desc->n_cov_extra > a.cov_extra_cap) a.desc->n_cov_extra = a.cov_extra_cap;
        // values for the message of the first failing read
        const unsigned long long key = a.err->first_key;
        if (key != BQC_ERRKEY_NONE) {
            const uint32_t i = (uint32_t)(key >> 3), order = (uint32_t)key & 7u;
            if (i < a.n) { a.err->aux0 = order == 1 ? a.l_seq[i] : order == 2 ? a.lane[i] : (uint32_t)a.rid[i]; a.err->aux1 = a.lane[i]; }
        }
    }
}

// entries of one super-window: read groups (first-mate slots | other slots, missing ones null), segment entries, generic reads.
// Thread t owns the positions [SC_PER * t, + SC_PER) of the super-window: their classes are requested together (two 16-byte loads
// in stream order), ranked by ONE workgroup scan of four counts, and placed from registers; the read groups leave LDS coalesced.
// (Round 5: a thread walked its positions twice, one dependent class load and store after another: latency-bound, 0.9 TB/s.)
#define SC_PER (BQC_SW_READS / PR_THREADS)
#define SC_ENT (3 * BQC_SW_READS + 128) // groups * rpw <= (count / h + 1) * rpw with rpw / h <= 2.5 (rpw = 5: 3 + 2 slots)
__global__ __launch_bounds__(PR_THREADS) void k_build_scatter(PrepArgs a)
{
    __shared__ uint32_t ent[SC_ENT];
    __shared__ uint32_t sh[4 * (PR_THREADS / 64)];
    const SuperWindow sw = a.sws[blockIdx.x];
    const SwPlan pl = a.sw_plan[blockIdx.x];
    const uint32_t fast_w = a.desc->fast_w, rpw = 64u / fast_w, h0 = (rpw + 1) / 2, h1 = rpw / 2;
    const uint32_t n_ent = pl.n_groups * rpw;
    if (n_ent > SC_ENT) { if (threadIdx.x == 0) atomicOr(&a.err->flags, BQC_DEVERR_INTERNAL); return; }
    for (uint32_t k = threadIdx.x; k < n_ent; k += PR_THREADS) ent[k] = 0xFFFFFFFFu;
    // the reads and their classes (class << 8 | segments; 3 << 8: no read)
    uint32_t r[SC_PER], v[SC_PER];
    const uint32_t p0 = SC_PER * threadIdx.x;
    if (!a.order && p0 + SC_PER <= sw.count && ((sw.begin + p0) & 7u) == 0u) {
        const uint4 x = *(const uint4*)(a.cls + sw.begin + p0), y = *(const uint4*)(a.cls + sw.begin + p0 + 8);
        const uint32_t wd[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
#pragma unroll
        for (int k = 0; k < SC_PER; ++k) { r[k] = sw.begin + p0 + k; v[k] = (wd[k >> 1] >> (16 * (k & 1))) & 0xFFFFu; }
    } else {
#pragma unroll
        for (int k = 0; k < SC_PER; ++k) { const uint32_t p = p0 + k; r[k] = p < sw.count ? (a.order ? a.order[sw.begin + p] : sw.begin + p) : 0xFFFFFFFFu; }
#pragma unroll
        for (int k = 0; k < SC_PER; ++k) v[k] = r[k] != 0xFFFFFFFFu ? a.cls[r[k]] : 3u << 8;
    }
    uint32_t c[4] = {0, 0, 0, 0}; // first-mate fast reads, other fast reads, generic reads, segment entries
#pragma unroll
    for (int k = 0; k < SC_PER; ++k) {
        const uint32_t cl = v[k] >> 8;
        c[0] += cl == 0u; c[1] += cl == 1u; c[2] += cl == 2u; c[3] += cl < 3u ? v[k] & 0xFFu : 0u;
    }
    uint32_t co[SC_PER]; // CIGAR offsets of the reads with segments (rare), requested before the scan
#pragma unroll
    for (int k = 0; k < SC_PER; ++k) co[k] = (v[k] >> 8) < 3u && (v[k] & 0xFFu) ? a.cigar_off[r[k]] : 0u;
    uint32_t tot[4];
    block_scan_excl_n<4>(c, sh, tot); // c: this thread's first ranks (its barriers also order the null entries before the placement)
    uint32_t k0 = c[0], k1 = c[1], k2 = c[2], k3 = c[3];
#pragma unroll
    for (int k = 0; k < SC_PER; ++k) {
        const uint32_t cl = v[k] >> 8, ns = v[k] & 0xFFu;
        if (cl == 0u) { ent[(k0 / h0) * rpw + k0 % h0] = r[k]; ++k0; }
        else if (cl == 1u) { ent[(k1 / h1) * rpw + h0 + k1 % h1] = r[k]; ++k1; }
        else if (cl == 2u) a.perm[pl.slow_base + k2++] = r[k];
        if (cl < 3u && ns) { for (uint32_t j = 0; j < ns; ++j) a.perm[pl.seg_base + k3 + j] = BQC_ENTRY_SEG | (co[k] + j); k3 += ns; }
    }
    block_sync();
    for (uint32_t k = threadIdx.x; k < n_ent; k += PR_THREADS) a.perm[pl.group_base + k] = ent[k];
}

// the unordered flags of the hot kernels and the keyed first error, for the host (one small copy per batch)
// after_reads (or nullptr): recorded behind k_prep_reads — cov[], cov_extra[] and desc->n_cov_extra are final there (k_cov's inputs)
extern "C" void bqc_launch_prep(const PrepArgs& a, const DevRefs& refs, hipStream_t s, hipEvent_t after_reads)
{
    if (a.n == 0) return;
    const uint32_t nblk = (a.n + PR_BLOCK - 1) / PR_BLOCK;
    hipLaunchKernelGGL(k_prep_sizes, dim3((nblk + PR_GROUP - 1) / PR_GROUP), dim3(PS_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_prep_reads, dim3(nblk), dim3(PR_THREADS), 0, s, a, refs);
    if (after_reads) (void)hipEventRecord(after_reads, s);
    if (a.order) hipLaunchKernelGGL(k_build_count, dim3(a.n_sw), dim3(PR_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_build_plan, dim3(1), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(k_build_scatter, dim3(a.n_sw), dim3(PR_THREADS), 0, s, a);
}

// The offsets' arithmetic on the host, step by step as the two kernels do it (tests: a batch with 4 GB of payload cannot be one).
extern "C" uint32_t bqc_prep_group(void) { return PR_GROUP; }
extern "C" uint32_t bqc_prep_bases(const uint64_t* blk_totals, uint32_t n_blocks, uint64_t* bases)
{
    const uint32_t n_groups = (n_blocks + PR_GROUP - 1) / PR_GROUP;
    std::vector<unsigned long long> blk(3ull * n_blocks), grp(3ull * n_groups);
    for (uint32_t g = 0; g < n_groups; ++g) // k_prep_sizes
        for (int k = 0; k < 3; ++k) {
            unsigned long long t = 0;
            for (uint32_t b = g * PR_GROUP; b < std::min(n_blocks, (g + 1) * PR_GROUP); ++b) { blk[3ull * b + k] = t; t += blk_totals[3ull * b + k]; }
            grp[3ull * g + k] = t;
        }
    uint32_t first_bad = 0xFFFFFFFFu;
    for (uint32_t b = 0; b < n_blocks; ++b) { // k_prep_reads
        const uint32_t g = b / PR_GROUP;
        const bool grp_last = (b + 1) % PR_GROUP == 0 || b + 1 == n_blocks;
        const unsigned long long* incl = grp_last ? &grp[3ull * g] : &blk[3ull * (b + 1)];
        unsigned long long before[3] = {0, 0, 0}, base[3];
        for (uint32_t g2 = 0; g2 < g; ++g2)
            for (int k = 0; k < 3; ++k) before[k] += grp[3ull * g2 + k];
        if (prep_block_bases(before, &blk[3ull * b], incl, base)) first_bad = std::min(first_bad, b);
        for (int k = 0; k < 3; ++k) bases[3ull * b + k] = base[k];
    }
    return first_bad;
}

// ---------------------------------------------------------------------------------------------------
// shard mode: the set-aside reads of a batch, once their windows are known
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pend_interval(uint32_t pos, uint32_t c0, uint32_t len) // off | len << 16 inside the read's two live windows, 0: nothing
{
    const uint32_t lo = pos + c0;
    if (!len || lo >= 2u * BQC_VSIZE) return 0u;
    const uint32_t hi = min(lo + len, 2u * BQC_VSIZE);
    return lo | ((hi - lo) << 16);
}
__global__ __launch_bounds__(256) void k_pend_cov(uint32_t n, const CovEntry* __restrict__ cov_in, const PendRun* __restrict__ pend, const PendExtra* __restrict__ extra,
                                                     const uint32_t* __restrict__ extra_n, uint32_t extra_cap, const uint8_t* __restrict__ lane,
                                                     CovEntry* __restrict__ cov_out, CovExtra* __restrict__ cov_extra, BatchDesc* __restrict__ desc)
{
    const uint32_t ne = min(*extra_n, extra_cap);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const CovEntry ce = cov_in[i];
        const PendRun r = pend[i];
        cov_out[i] = CovEntry{ce.win, pend_interval(ce.off_len, r.c0, r.len)};
    }
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += gridDim.x * blockDim.x) {
        const PendExtra x = extra[e];
        const CovEntry ce = cov_in[x.idx];
        cov_extra[e] = CovExtra{ce.win, pend_interval(ce.off_len, x.c0, x.len), lane[x.idx], 0};
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { desc->n_cov_extra = ne; desc->fatal = 0; }
}
extern "C" void bqc_launch_pend_cov(uint32_t n, const CovEntry* cov_in, const PendRun* pend, const PendExtra* extra, const uint32_t* extra_n, uint32_t extra_cap,
                                    const uint8_t* lane, CovEntry* cov_out, CovExtra* cov_extra, BatchDesc* desc, hipStream_t s)
{
    if (!n) return;
    hipLaunchKernelGGL(k_pend_cov, dim3(std::min<uint32_t>((n + 255) / 256, 4096u)), dim3(256), 0, s, n, cov_in, pend, extra, extra_n, extra_cap, lane, cov_out, cov_extra, desc);
}
