// k_gcb.hip — GC bias (--gc-bias; the statistic: include/bamqc.h): G[g] counts the genome's windows of W bases by
// their GC bin, R[lane][g] the counted reads by the bin of the window they start in, B and Q their bases and the sum of their quality
// bytes.  An optional module beside k_qcyc, k_mbc and k_adp: its launches exist only after bqc_enable_gc_bias.
//
// Both kernels count four Dna5 codes at once: (x ^ (x >> 1)) & 0x01010101 marks C and G (codes 1, 2), (x >> 2) & 0x01010101 marks N
// (code 4); a pair of counts travels as gc | n << 16.  The bin floor(100 gc / (W - n)) has five divisors per launch: GcbDiv holds their
// reciprocals (device_types.h), the quotient is one __umulhi.  Neither kernel touches a byte outside [0, len) of a contig or outside a
// read's quality bytes other than through the aligned dwords that hold at least one wanted byte.
//
// k_gcb_genome.  A share is GG_SHARE consecutive window starts of one contig; the workgroups take shares round robin (the contig of a
// share: a binary search in the table of first shares).  The share's bytes — GG_SHARE + W - 1 at most, from any byte alignment — come in
// as aligned dwords, coalesced, into LDS; thread t counts dwords GG_ITEMS t .. + GG_ITEMS - 1 (GG_ITEMS odd: the threads' runs begin in
// distinct banks), the block scans the 256 sums (DPP within a wave, four wave totals through LDS), and every dword gets the count of
// the bytes in front of it.  A window start is then two lookups: counts in front of byte s + W minus counts in front of byte s, each a
// prefix word and the masked dword itself.  Consecutive lanes take consecutive starts: four lanes share a dword, no bank conflict.
// Neighbouring windows differ by one base, so a wave's 64 starts fall into a handful of bins: equal bins are counted by ballot and added
// once, to a histogram in LDS that the workgroup keeps over all its shares and adds to G at the end (non-zero bins only).  The
// histogram is u32: the launch gives a workgroup fewer than 2^18 shares of 2^13 starts.
//
// k_gcb_reads.  About one workgroup per CU; a workgroup takes a contiguous share of the batch's processing order, GR_STEP reads at a
// time, thread t of a step fetching the columns of the step's read t (and those of the next step before this one is counted): it
// applies the rule, walks the CIGAR of a reverse read (64-bit sum of the reference-consuming lengths) and leaves the window's address,
// the quality bytes' offset and their number (0 for a read without qualities) in LDS.  A read then gets a power of two of lanes, chosen
// from the step's longest read and W (16 bytes a lane: 16 lanes at 150 bases, four reads per wave instruction); lane j takes the
// aligned dwords j, j + w, ... of the window and of the qualities, first and last masked; the quality bytes are summed by v_sad_u8
// into 64 bits; the lanes of a read meet by shuffles.  The read's first lane adds to a tile of 3 x 101 u64 in LDS (64-bit LDS
// atomics: B and Q cannot overflow).  The tile belongs to one read group at a time — the lowest of the step's — and is flushed when
// that changes and at the end; a counted read of another read group (only a step that spans a change holds one) goes to device memory.
#include <algorithm>
#include "kernels_common.h"
#include "cigar_walk.h" // share_grid: the launch geometry of a kernel that shares the reads out

#define GG_THREADS 256
#define GG_ITEMS 9                   // dwords a thread counts for the scan (odd)
#define GG_ND (GG_THREADS * GG_ITEMS) // dwords of a share's bytes the LDS holds
#define GG_SHARE 8192                // window starts of a share
#define GG_WG_SHARES (1u << 18)      // a workgroup takes fewer shares than this (its histogram is u32)
#define GR_THREADS 1024
#define GR_WAVES (GR_THREADS / WAVE)
#define GR_STEP GR_THREADS           // reads whose columns a workgroup fetches at a time, one per thread
#define GR_TILE (BQC_GCB_ROWS * BQC_GCB_BINS)
#define GCB_NOBIN 0xFFFFFFFFu
#define GR_NOLANE 0xFFFFFFFFu

// the share's dwords: up to 3 bytes in front of its first, GG_SHARE + W - 1 bytes, up to 3 behind, and the one word behind them all
static_assert((3 + GG_SHARE + BQC_GCB_WMAX - 1 + 3) / 4 + 1 <= GG_ND, "a share's bytes must fit the LDS image");
static_assert(GG_ITEMS % 2 == 1 && GG_SHARE % GG_THREADS == 0, "");
static_assert(4ull * GG_ND < 65536, "a share's packed counts stay below 2^16");

// gc | n << 16 of the bytes of x that bm selects (a subset of 0x01010101)
__device__ __forceinline__ uint32_t gcb_cnt(uint32_t x, uint32_t bm)
{
    return (uint32_t)__popc((x ^ (x >> 1)) & bm) | (uint32_t)__popc((x >> 2) & bm) << 16;
}

// the bin of a window with the counts c = gc | n << 16 (GCB_NOBIN: more than four N)
__device__ __forceinline__ uint32_t gcb_bin(uint32_t c, const GcbDiv& D)
{
    const uint32_t gc = c & 0xFFFFu, n = c >> 16;
    if (n > 4u) return GCB_NOBIN;
    const uint32_t m = n == 0u ? D.m[0] : n == 1u ? D.m[1] : n == 2u ? D.m[2] : n == 3u ? D.m[3] : D.m[4];
    return __umulhi(100u * gc, m);
}

__global__ __launch_bounds__(GG_THREADS) void k_gcb_genome(const GcbContig* __restrict__ tab, uint32_t n_contigs, uint64_t n_shares, uint32_t W, GcbDiv D, uint64_t* __restrict__ G)
{
    __shared__ uint32_t s_raw[GG_ND], s_pre[GG_ND], s_hist[128], s_wsum[GG_THREADS / WAVE];
    const uint32_t tid = threadIdx.x, wave = tid / WAVE, ln = lane_id();
    if (tid < 128u) s_hist[tid] = 0; // (in front of the first share's barriers)
    for (uint64_t sh = blockIdx.x; sh < n_shares; sh += gridDim.x) {
        uint32_t lo = 0, hi = n_contigs; // the last contig whose first share is at or before sh (tab[0].share0 = 0)
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (tab[mid].share0 <= sh) lo = mid; else hi = mid;
        }
        const GcbContig ct = tab[lo];
        const uint64_t s0 = (sh - ct.share0) * GG_SHARE; // (< nstarts: the contig has a share for it)
        const uint32_t ns = (uint32_t)min((uint64_t)GG_SHARE, ct.nstarts - s0);
        // wanted bytes: [s0, s0 + ns + W - 1), all inside [0, len) since s0 + ns <= len - W + 1
        const uintptr_t a0 = (uintptr_t)ct.ref + s0;
        const uint32_t o = (uint32_t)a0 & 3u, nd = (o + ns + W - 1u + 3u) >> 2; // (every one of the nd dwords holds a wanted byte)
        const gmem_u32* src = (const gmem_u32*)(a0 & ~(uintptr_t)3);
        for (uint32_t k = tid; k < GG_ND; k += GG_THREADS) s_raw[k] = k < nd ? src[k] : 0u;
        block_sync();
        uint32_t cnt[GG_ITEMS], sum = 0;
#pragma unroll
        for (uint32_t i = 0; i < GG_ITEMS; ++i) { cnt[i] = gcb_cnt(s_raw[tid * GG_ITEMS + i], 0x01010101u); sum += cnt[i]; }
        const uint32_t incl = wave_scan_incl(sum); // (both halves of the packed sums stay below 2^16: no carry between them)
        if (ln == WAVE - 1) s_wsum[wave] = incl;
        block_sync();
        uint32_t run = incl - sum;
        for (uint32_t w = 0; w < wave; ++w) run += s_wsum[w];
#pragma unroll
        for (uint32_t i = 0; i < GG_ITEMS; ++i) { s_pre[tid * GG_ITEMS + i] = run; run += cnt[i]; }
        block_sync();
        for (uint32_t i0 = 0; i0 < ns; i0 += GG_THREADS) { // (ns is the workgroup's: the ballots below see whole waves)
            const uint32_t i = i0 + tid;
            uint32_t g = GCB_NOBIN;
            if (i < ns) {
                const uint32_t b0 = o + i, b1 = b0 + W; // bytes of the image; b1 <= 4 nd, and word nd of both arrays is there (zero bytes)
                const uint32_t c1 = s_pre[b1 >> 2] + gcb_cnt(s_raw[b1 >> 2], 0x01010101u & ((1u << (8u * (b1 & 3u))) - 1u));
                const uint32_t c0 = s_pre[b0 >> 2] + gcb_cnt(s_raw[b0 >> 2], 0x01010101u & ((1u << (8u * (b0 & 3u))) - 1u));
                g = gcb_bin(c1 - c0, D); // (each half of c1 is at least that of c0: no borrow)
            }
            uint64_t m = __ballot(g != GCB_NOBIN);
            while (m) {
                const int leader = __ffsll((unsigned long long)m) - 1;
                const uint32_t g0 = __builtin_amdgcn_readlane(g, leader);
                const uint64_t sm = __ballot(g == g0);
                if ((int)ln == leader) atomicAdd(&s_hist[g0], (uint32_t)__popcll((unsigned long long)sm));
                m &= ~sm;
            }
        }
        block_sync(); // (the image is read to here)
    }
    block_sync();
    if (tid < BQC_GCB_BINS && s_hist[tid]) gadd(G + tid, s_hist[tid]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Read i of the processing order: the address of its window's first genome byte, its quality bytes, its read group (GR_NOLANE: the read
// is not counted, or only its bin is still open — a window without a bin is found when its bytes are counted)
struct GrRead { uint64_t wa; uint32_t qoff, lq, lane; };
__device__ __forceinline__ GrRead gr_fetch(const DevBatch& b, const DevRefs& refs, uint64_t i, uint32_t end, uint32_t W, uint32_t n_lanes)
{
    GrRead o{0ull, 0u, 0u, GR_NOLANE};
    if (i >= end) return o;
    const uint32_t r = b.order ? b.order[i] : (uint32_t)i;
    if (r >= b.n_reads) return o;
    const uint32_t f = b.flag[r], g = b.lane[r], nc = b.n_cigar[r];
    const int32_t rid = b.rid[r];
    if ((f & 0x904u) || !nc || g >= n_lanes || rid < 0 || (uint32_t)rid >= refs.n_refs) return o;
    const uint8_t* ref = refs.ref[rid];
    if (!ref) return o;
    int64_t s = b.pos[r];
    if (f & 0x10u) { // reverse: the window ends where the alignment ends
        const uint32_t* cg = b.cigar + b.cigar_off[r];
        int64_t span = 0;
        for (uint32_t k = 0; k < nc; ++k) {
            const uint32_t wd = cg[k];
            if ((0x18Du >> (wd & 15u)) & 1u) span += (int64_t)(wd >> 4); // M, D, N, =, X
        }
        s += span - (int64_t)W;
    }
    if (s < 0 || (uint64_t)s + W > refs.len[rid]) return o;
    o.wa = (uint64_t)(uintptr_t)ref + (uint64_t)s;
    o.lane = g;
    if (!(f & BQC_FLAG_NO_QUAL)) { o.lq = b.l_seq[r]; o.qoff = b.qual_off[r]; }
    return o;
}

// the bytes [o, o + n) of an image of aligned dwords that dword k holds, as a mask of whole bytes (k < ceil((o + n) / 4), o < 4)
__device__ __forceinline__ uint32_t gr_bytes(uint32_t k, uint32_t o, uint64_t n)
{
    uint32_t m = k ? 0xFFFFFFFFu : 0xFFFFFFFFu << (8u * o);
    const uint64_t left = o + n - 4ull * k; // bytes from the dword's first to the end of the range (>= 1)
    if (left < 4ull) m &= (1u << (8u * (uint32_t)left)) - 1u;
    return m;
}

// tile -> the words of read group `lane`, and the tile back to zero
__device__ __forceinline__ void gr_flush(unsigned long long* tile, uint64_t* __restrict__ tab, uint32_t lane)
{
    block_sync();
    for (uint32_t t = threadIdx.x; t < GR_TILE; t += GR_THREADS) {
        const unsigned long long v = tile[t];
        if (!v) continue;
        tile[t] = 0;
        gadd(tab + (uint64_t)lane * GR_TILE + t, v);
    }
    block_sync();
}

__global__ __launch_bounds__(GR_THREADS) void k_gcb_reads(DevBatch b, DevRefs refs, uint64_t* __restrict__ tab, uint32_t W, GcbDiv D, uint32_t n_lanes, uint32_t per)
{
    __shared__ unsigned long long tile[GR_TILE + 1];
    __shared__ uint32_t s_alo[GR_STEP], s_ahi[GR_STEP], s_qoff[GR_STEP], s_lq[GR_STEP], s_lane[GR_STEP];
    __shared__ uint32_t s_mm[2]; // [0] the lowest read group of the step's reads that passed the rule, [1] their longest run of quality bytes
    if (b.desc->fatal) return;
    const uint32_t tid = threadIdx.x, wave = tid / WAVE, ln = lane_id();
    const uint64_t begin64 = (uint64_t)blockIdx.x * per;
    if (begin64 >= b.n_reads) return;
    const uint32_t begin = (uint32_t)begin64, end = (uint32_t)min((uint64_t)b.n_reads, begin64 + per);
    for (uint32_t t = tid; t < GR_TILE; t += GR_THREADS) tile[t] = 0;
    uint32_t tile_lane = GR_NOLANE;
    GrRead nx = gr_fetch(b, refs, (uint64_t)begin + tid, end, W, n_lanes);
    for (uint32_t base = begin; base < end; base += GR_STEP) {
        const GrRead me = nx;
        if (end - base > GR_STEP) nx = gr_fetch(b, refs, (uint64_t)base + GR_STEP + tid, end, W, n_lanes); // (in flight while this step is counted)
        s_alo[tid] = (uint32_t)me.wa; s_ahi[tid] = (uint32_t)(me.wa >> 32); s_qoff[tid] = me.qoff; s_lq[tid] = me.lq; s_lane[tid] = me.lane;
        if (tid == 0) { s_mm[0] = GR_NOLANE; s_mm[1] = 0; }
        block_sync();
        if (me.lane != GR_NOLANE) { atomicMin(&s_mm[0], me.lane); atomicMax(&s_mm[1], me.lq); }
        block_sync();
        const uint32_t cur = s_mm[0], longest = max(s_mm[1], W);
        if (cur != GR_NOLANE) {
            if (cur != tile_lane) {
                if (tile_lane != GR_NOLANE) gr_flush(tile, tab, tile_lane);
                tile_lane = cur;
            }
            const uint32_t nstep = min((uint32_t)GR_STEP, end - base);
            const uint32_t chunks = (longest >> 4) + ((longest & 15u) ? 1u : 0u);
            const uint32_t lg = chunks >= 64u ? 6u : chunks <= 1u ? 0u : 32u - (uint32_t)__clz((int)(chunks - 1u)); // lanes per read: 1 << lg
            const uint32_t w = 1u << lg, rp = 64u >> lg, sub = ln >> lg, j = ln & (w - 1u);
            for (uint32_t g0 = wave * rp; g0 < nstep; g0 += GR_WAVES * rp) { // (the wave's: the shuffles below see whole groups of lanes)
                const uint32_t g = g0 + sub;
                const uint32_t lane = g < nstep ? s_lane[g] : GR_NOLANE;
                uint32_t c = 0;
                uint64_t qs = 0;
                uint32_t lq = 0;
                if (lane != GR_NOLANE) {
                    const uintptr_t wa = (uintptr_t)((uint64_t)s_ahi[g] << 32 | s_alo[g]);
                    const uint32_t o = (uint32_t)wa & 3u, nd = (o + W + 3u) >> 2;
                    const gmem_u32* src = (const gmem_u32*)(wa & ~(uintptr_t)3);
                    for (uint32_t k = j; k < nd; k += w) c += gcb_cnt(src[k], gr_bytes(k, o, W) & 0x01010101u);
                    lq = s_lq[g];
                    if (lq) {
                        const uintptr_t qa = (uintptr_t)(b.qual + s_qoff[g]);
                        const uint32_t qo = (uint32_t)qa & 3u;
                        const uint64_t nq = ((uint64_t)qo + lq + 3ull) >> 2;
                        const gmem_u32* qsrc = (const gmem_u32*)(qa & ~(uintptr_t)3);
                        for (uint64_t k = j; k < nq; k += w) qs += __builtin_amdgcn_sad_u8(qsrc[k] & gr_bytes((uint32_t)k, qo, lq), 0u, 0u);
                    }
                }
                for (uint32_t off = 1; off < w; off <<= 1) {
                    c += __shfl_xor(c, (int)off);
                    qs += __shfl_xor((unsigned long long)qs, (int)off);
                }
                const uint32_t bin = lane != GR_NOLANE && !j ? gcb_bin(c, D) : GCB_NOBIN; // (the read's first lane adds)
                if (bin == GCB_NOBIN) continue;
                if (lane == cur) {
                    atomicAdd(&tile[bin], 1ull);
                    if (lq) { atomicAdd(&tile[BQC_GCB_BINS + bin], (unsigned long long)lq); atomicAdd(&tile[2 * BQC_GCB_BINS + bin], (unsigned long long)qs); }
                } else {
                    uint64_t* tl = tab + (uint64_t)lane * GR_TILE + bin;
                    gadd(tl, 1);
                    if (lq) { gadd(tl + BQC_GCB_BINS, lq); gadd(tl + 2 * BQC_GCB_BINS, qs); }
                }
            }
        }
        block_sync(); // (the step's columns are read to here)
        if (end - base <= GR_STEP) break; // (not left to the loop's test: base + GR_STEP may wrap)
    }
    if (tile_lane != GR_NOLANE) gr_flush(tile, tab, tile_lane);
}

extern "C" uint64_t bqc_gcb_words(uint32_t n_lanes) { return (uint64_t)n_lanes * GR_TILE; }
extern "C" uint32_t bqc_gcb_share(void) { return GG_SHARE; }

// G += the windows of the n_contigs contigs of `tab` (device memory; n_shares = the shares of all of them, at least one)
extern "C" void bqc_launch_gcb_genome(const GcbContig* tab, uint32_t n_contigs, uint64_t n_shares, uint32_t W, const GcbDiv& D, uint64_t* G, uint32_t n_cu, hipStream_t s)
{
    if (!n_contigs || !n_shares) return;
    // eight workgroups a CU (18.5 KiB of LDS each), more where a workgroup would otherwise take GG_WG_SHARES shares or more
    const uint64_t least = n_shares / (GG_WG_SHARES - 1u) + 1u;
    const uint64_t grid = std::min(n_shares, std::max<uint64_t>((uint64_t)n_cu * 8u, least));
    hipLaunchKernelGGL(k_gcb_genome, dim3((uint32_t)grid), dim3(GG_THREADS), 0, s, tab, n_contigs, n_shares, W, D, G);
}

// workgroups: about one per CU, a small batch gets fewer; each takes `per` consecutive reads of the processing order
extern "C" void bqc_launch_gcb_reads(const DevBatch& b, const DevRefs& refs, uint64_t* tab, uint32_t W, const GcbDiv& D, uint32_t n_lanes, uint32_t n_cu, hipStream_t s)
{
    if (b.n_reads == 0) return;
    uint32_t per;
    const uint32_t g = share_grid(b.n_reads, n_cu, &per);
    hipLaunchKernelGGL(k_gcb_reads, dim3(g), dim3(GR_THREADS), 0, s, b, refs, tab, W, D, n_lanes, per);
}
