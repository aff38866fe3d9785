// k_sbc.hip — substitutions by sequence context and by cycle (--substitutions; the statistic: include/bamqc.h):
// X[lane][mate][strand][context][read base] and Y[lane][mate][cycle][genome base][read base], both as sequenced, over the examined
// pairs of base quality >= Q in reads of mapping quality >= MQ.  An optional module beside k_mbc: its launch exists only after
// bqc_enable_substitutions.
//
// Mapping.  k_mbc's (mbc_walk.h, k_mbc.hip): about one workgroup per CU, SB_WAVES waves, SB_STEP reads at a time; a thread walks the
// CIGAR of its read into RUNS of stored positions in an LDS list, consumed in rounds; a wave takes one run per instruction, lane j the
// stored bases start + 4j .. + 3, runs of more than 256 positions in further passes; the loads of SB_U runs are requested together.
// The genome window.  A lane needs the genome bytes of its positions and of one neighbour on either side: up to six bytes at any
// alignment, one to three aligned dwords (sb_gload).  Inside a run the neighbour is a byte of the run; at a run's first and last
// position it exists iff it is a byte of [0, len) of the contig — two bits of the run's info word, set where the run is made — and a
// neighbour that does not exist is "no context", never a load.  Only dwords that hold a byte of [0, len) are touched.
// Y.  [2 mates][16 bins][C cycles] u32 in LDS, the cycle swizzled as in k_qcyc and k_mbc: the 64 lanes of an LDS atomic hold 64
// cycles four apart of one read, which fall on 64 consecutive words whatever bin each lane counts.  Cycles at or behind C go to
// device memory with one global atomic each.
// X.  More than 99 % of the pairs of real data are matches, and a run's matches have at most 64 addresses (the diagonal bins of its
// mate and strand).  A table per wave, [2 mates][2 strands][64][4] u32 (4 KiB) summed at the flush, was built first and measured
// against ONE table for the workgroup: the same time within 1 % on both shapes — the CU's LDS serves one wave's
// atomic at a time whichever table it goes to, and what queues is the lanes of ONE instruction on equal addresses.  So the kernel
// keeps the one table, and the 60 KiB go to Y: C = SB_C = 1024 cycles, the program's default capacity, instead of 512.
// (BQC_SBC_X, read once per process, selects the measured alternatives for tools/sbc_time.py: 1 = one table, C = 512; 2 = a table
// per wave, C = 512.)  Mismatches take the same path.
// The tiles belong to one read group at a time and are flushed (non-zero bins only) when the read group changes, at the end, and before
// the positions listed since the last flush could reach 2^32: a bin takes at most one addition per listed position.
#include <algorithm>
#include <cstdlib>
#include "kernels_common.h"
#include "mbc_walk.h"

#define SB_THREADS 1024
#define SB_WAVES (SB_THREADS / WAVE)
#define SB_C 1024                    // cycles of Y the tile holds
#define SB_C_ALT 512                 // ... in the measured alternatives, where the tables X take up to 64 KiB
#define SB_XT (2 * 2 * 64 * 4)       // a table X: one per wave, or one for all
#define SB_U 4                       // runs whose loads a wave requests together
#define SB_STEP 768                  // reads whose columns a workgroup fetches at a time
#define SB_RUNS 768                  // runs the list holds
#define SB_RW 8                      // words of a run
#define SB_NOLANE 0xFFFFFFFFu
#define SB_LEFT (1u << 10)           // info: the genome has a byte in front of the run's first position
#define SB_RIGHT (1u << 11)          //       and one behind its last
#define SB_LDS_WORDS(xc, c) (2 * 16 * (c) + (xc) * SB_XT + SB_RW * SB_RUNS + 8)

template <uint32_t C> __device__ __forceinline__ uint32_t sb_swz(uint32_t c) { return (c & 3u) * (C / 4) + (c >> 2); }

// the bytes at the addresses [a_lo, a_hi] (a_hi - a_lo <= 5), byte a_lo lowest, from the one to three aligned dwords that hold them.
// Only dwords that hold one of those bytes are touched.
__device__ __forceinline__ uint64_t sb_gload(uintptr_t a_lo, uintptr_t a_hi)
{
    const gmem_u32* a = (const gmem_u32*)(a_lo & ~(uintptr_t)3);
    const uint32_t nd = (uint32_t)(((a_hi & ~(uintptr_t)3) - (a_lo & ~(uintptr_t)3)) >> 2);
    const uint32_t w0 = a[0];
    uint32_t w1 = 0, w2 = 0;
    if (nd >= 1u) w1 = a[1];
    if (nd >= 2u) w2 = a[2];
    const uint32_t sh = 8u * (uint32_t)(a_lo & 3u);
    uint64_t v = ((uint64_t)w1 << 32 | w0) >> sh;
    if (sh) v |= (uint64_t)w2 << (64u - sh);
    return v;
}

// What a lane holds of a run: its stored positions [lo, hi) (at most four; lo >= hi: none), their qualities and nibbles as in k_mbc,
// and the genome bytes from the left neighbour of lo (left = 1) or from lo itself (left = 0) on, in wg.
struct SbReq { uint32_t lo, hi, L, info, left, right; uintptr_t qa, sa; uint64_t wq, ws, wg; };

// tl: the words of the read group — [2 mates]{X [2][64][4], Y [N][16]}
template <uint32_t C> __device__ __forceinline__ void sb_count(const SbReq& q, uint32_t* ytile, uint32_t* xt, uint64_t* __restrict__ tl, uint32_t N, uint32_t Q)
{
    const uint32_t mate = (q.info >> 8) & 1u;
    const uint32_t rev = (q.info >> 9) & 1u;
    uint64_t* Yg = tl + (uint64_t)mate * BQC_SBC_MATE_WORDS(N) + BQC_SBC_X_WORDS;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t p = q.lo + k;
        if (p >= q.hi) break;
        const uint32_t ql = mb_byte(q.wq, q.qa, k);
        const uint32_t sb = mb_byte(q.ws, q.sa, (p >> 1) - (q.lo >> 1));
        const uint32_t nib = (p & 1u) ? sb & 15u : sb >> 4;
        const uint32_t gi = k + q.left;                        // the byte of p in wg
        const uint32_t gc = (uint32_t)(q.wg >> (8u * gi)) & 255u;
        const uint32_t c = rev ? q.L - 1u - p : p;             // sequencing orientation
        if (!nib || (nib & (nib - 1u)) || gc > 3u || ql > 222u || ql < Q || c >= N) continue;
        const uint32_t gl = gi ? (uint32_t)(q.wg >> (8u * (gi - 1u))) & 255u : 4u;                   // (gi = 0: the run's first position without a byte in front)
        const uint32_t gr = (p + 1u < q.hi || q.right) ? (uint32_t)(q.wg >> (8u * (gi + 1u))) & 255u : 4u;
        uint32_t bb = (uint32_t)__ffs((int)nib) - 1u, t = gc;
        if (rev) { bb = 3u - bb; t = 3u - t; }
        const uint32_t bin = t * 4u + bb;
        if (c < C) atomicAdd(&ytile[(mate * 16u + bin) * C + sb_swz<C>(c)], 1u);
        else gadd(Yg + (uint64_t)c * 16u + bin, 1);
        if (gl <= 3u && gr <= 3u) {
            const uint32_t ctx = rev ? 16u * (3u - gr) + 4u * t + (3u - gl) : 16u * gl + 4u * t + gr;
            atomicAdd(&xt[((mate * 2u + rev) * 64u + ctx) * 4u + bb], 1u);
        }
    }
}

// tiles -> the words of read group `lane`, and the tiles back to zero.  xc: the tables X there are.
template <uint32_t C> __device__ __forceinline__ void sb_flush(uint32_t* ytile, uint32_t* x, uint32_t xc, uint64_t* __restrict__ tables, uint32_t lane, uint32_t N)
{
    block_sync();
    const uint64_t mw = BQC_SBC_MATE_WORDS(N);
    uint64_t* tl = tables + (uint64_t)lane * 2 * mw;
    for (uint32_t t = threadIdx.x; t < 2 * 16 * C; t += SB_THREADS) {
        const uint32_t v = ytile[t];
        if (!v) continue;
        ytile[t] = 0;
        const uint32_t mate = t / (16 * C), bin = (t / C) & 15u, pos = t % C, c = (pos & (C / 4 - 1)) * 4u + pos / (C / 4);
        if (c < N) gadd(tl + mate * mw + BQC_SBC_X_WORDS + (uint64_t)c * 16u + bin, v); // (a non-zero bin has c < N: said again where the address is made)
    }
    for (uint32_t t = threadIdx.x; t < SB_XT; t += SB_THREADS) { // t = (mate * 2 + strand) * 256 + ctx * 4 + base
        uint64_t v = 0;
        for (uint32_t w = 0; w < xc; ++w) {
            const uint32_t u = x[w * SB_XT + t];
            if (u) { v += u; x[w * SB_XT + t] = 0; }
        }
        if (v) gadd(tl + (uint64_t)(t >> 9) * mw + (t & 511u), v);
    }
    block_sync();
}

template <uint32_t XC, uint32_t C> // the tables X: 1, or SB_WAVES (one per wave); the cycles of the tile
__global__ __launch_bounds__(SB_THREADS) void k_sbc(DevBatch b, DevRefs refs, uint64_t* __restrict__ tables, uint32_t N, uint32_t Q, uint32_t MQ, uint32_t n_lanes)
{
    extern __shared__ uint32_t lds[];
    if (b.desc->fatal) return;
    uint32_t* ytile = lds;
    uint32_t* x = lds + 2 * 16 * C;
    uint32_t* s_qoff = x + XC * SB_XT;
    uint32_t* s_soff = s_qoff + SB_RUNS;
    uint32_t* s_ia = s_soff + SB_RUNS;
    uint32_t* s_ib = s_ia + SB_RUNS;
    uint32_t* s_L = s_ib + SB_RUNS;
    uint32_t* s_galo = s_L + SB_RUNS;
    uint32_t* s_gahi = s_galo + SB_RUNS;
    uint32_t* s_info = s_gahi + SB_RUNS;
    uint32_t* s_ctl = s_info + SB_RUNS; // [0] slots asked for, [1] a thread found the list full, [2] lowest, [3] highest read group of the list, [4] the next one, [6..7] the listed positions (u64)
    unsigned long long* s_npos = (unsigned long long*)(s_ctl + 6); // (an even word of the array: 8-byte aligned)
    const uint32_t tid = threadIdx.x, wave = tid / WAVE, ln = lane_id();
    uint32_t* xt = x + (XC > 1 ? wave * SB_XT : 0u);
    const uint32_t per = (uint32_t)(((uint64_t)b.n_reads + gridDim.x - 1) / gridDim.x);
    const uint64_t begin64 = (uint64_t)blockIdx.x * per;
    if (begin64 >= b.n_reads) return;
    const uint32_t begin = (uint32_t)begin64, end = (uint32_t)min((uint64_t)b.n_reads, begin64 + per);
    for (uint32_t t = tid; t < 2 * 16 * C + XC * SB_XT; t += SB_THREADS) lds[t] = 0;
    uint32_t tile_lane = SB_NOLANE;
    uint64_t since = 0; // positions listed since the tiles were last zero: what a bin can hold at most
    MbWalk w;
    for (uint32_t base = begin; base < end; base += SB_STEP) {
        const uint64_t i = tid < SB_STEP ? (uint64_t)base + tid : ~0ull;
        mb_fetch(w, b, refs, i, end, N, n_lanes);
        if (w.nc) { // .mbc's conditions hold; in addition mapq >= MQ
            const uint32_t r = b.order ? b.order[i] : (uint32_t)i;
            if (b.mapq[r] < MQ) w.k = w.nc = 0;
        }
        bool have = mb_next(w, b.cigar);
        for (;;) { // rounds of the step: one, unless its reads have more runs than the list holds
            if (tid == 0) { s_ctl[0] = 0; s_ctl[1] = 0; s_ctl[2] = SB_NOLANE; s_ctl[3] = 0; *s_npos = 0ull; }
            block_sync();
            while (have) {
                const uint32_t slot = atomicAdd(&s_ctl[0], 1u);
                if (slot >= SB_RUNS) { s_ctl[1] = 1u; break; } // (full: this run waits for the next round)
                const int64_t posv = (int64_t)(w.ga - w.ref);  // the genome position of stored position 0
                uint32_t info = w.info;
                if (posv + (int64_t)w.ia >= 1) info |= SB_LEFT;
                if (posv + (int64_t)w.ib < (int64_t)w.len) info |= SB_RIGHT;
                s_qoff[slot] = w.qoff; s_soff[slot] = w.soff; s_ia[slot] = w.ia; s_ib[slot] = w.ib; s_L[slot] = w.L;
                s_galo[slot] = (uint32_t)w.ga; s_gahi[slot] = (uint32_t)((uint64_t)w.ga >> 32); s_info[slot] = info;
                atomicMin(&s_ctl[2], w.info & 255u);
                atomicMax(&s_ctl[3], w.info & 255u);
                atomicAdd(s_npos, (unsigned long long)(w.ib - w.ia));
                have = mb_next(w, b.cigar);
            }
            block_sync();
            const uint32_t n = min(s_ctl[0], (uint32_t)SB_RUNS);
            const bool more = s_ctl[1] != 0u;
            uint32_t cur = s_ctl[2];
            const uint32_t last = s_ctl[3];
            const uint64_t npos = *s_npos;
            if (tile_lane != SB_NOLANE && since + npos > 0xFFFFFFFFull) { // (uniform: every thread reads the same words)
                sb_flush<C>(ytile, x, XC, tables, tile_lane, N);
                since = 0;
            }
            since += npos;
            while (cur != SB_NOLANE) { // one pass per read group the list holds: one, unless the step spans a change of read group
                if (cur != tile_lane) {
                    if (tile_lane != SB_NOLANE) { sb_flush<C>(ytile, x, XC, tables, tile_lane, N); since = npos; }
                    tile_lane = cur;
                }
                uint64_t* tl = tables + (uint64_t)cur * 2 * BQC_SBC_MATE_WORDS(N);
                // lane ln's part of pass `it` (256 stored positions a pass) of run e; runs behind n or of another read group: nothing
                auto request = [&](uint32_t e, uint32_t it) {
                    SbReq q;
                    q.lo = q.hi = 0;
                    if (e >= n) return q;
                    q.info = s_info[e];
                    if ((q.info & 255u) != cur) return q;
                    const uint32_t ia = s_ia[e], ib = s_ib[e];
                    const uint64_t off = (uint64_t)(ia & ~3u) + 256ull * it + 4u * ln;
                    if (off >= ib) return q;
                    q.lo = max((uint32_t)off, ia);
                    q.hi = (uint32_t)min(off + 4u, (uint64_t)ib);
                    q.L = s_L[e];
                    q.left = (q.lo > ia || (q.info & SB_LEFT)) ? 1u : 0u;   // the byte in front of lo: of the run, or of the contig
                    q.right = (q.hi < ib || (q.info & SB_RIGHT)) ? 1u : 0u; // the byte behind hi - 1
                    q.qa = (uintptr_t)(b.qual + s_qoff[e]) + q.lo;
                    q.sa = (uintptr_t)(b.seq + s_soff[e]) + (q.lo >> 1);
                    const uintptr_t ga = (uintptr_t)((uint64_t)s_gahi[e] << 32 | s_galo[e]) + q.lo;
                    q.wq = mb_load(q.qa, q.qa + (q.hi - 1u - q.lo));
                    q.ws = mb_load(q.sa, q.sa + (((q.hi - 1u) >> 1) - (q.lo >> 1)));
                    q.wg = sb_gload(ga - q.left, ga + (q.hi - 1u - q.lo) + q.right); // every byte of it one of [0, len)
                    return q;
                };
                for (uint32_t e0 = wave * SB_U; e0 < n; e0 += SB_WAVES * SB_U) {
                    SbReq q[SB_U];
#pragma unroll
                    for (int u = 0; u < SB_U; ++u) q[u] = request(e0 + u, 0);
#pragma unroll
                    for (int u = 0; u < SB_U; ++u) sb_count<C>(q[u], ytile, xt, tl, N, Q);
#pragma unroll
                    for (int u = 0; u < SB_U; ++u) { // runs of more than 256 positions (ia rounded down included): further passes
                        if (e0 + u >= n) break;
                        const uint32_t span = s_ib[e0 + u] - (s_ia[e0 + u] & ~3u);
                        for (uint32_t it = 1; it < (span + 255u) / 256u; ++it) sb_count<C>(request(e0 + u, it), ytile, xt, tl, N, Q);
                    }
                }
                if (cur == last) break;
                block_sync();
                if (tid == 0) s_ctl[4] = SB_NOLANE;
                block_sync();
                if (tid < n && (s_info[tid] & 255u) > cur) atomicMin(&s_ctl[4], s_info[tid] & 255u);
                block_sync();
                cur = s_ctl[4];
            }
            block_sync(); // (the list is read to here)
            if (!more) break;
        }
        if (end - base <= SB_STEP) break; // (not left to the loop's test: base + SB_STEP may wrap)
    }
    if (tile_lane != SB_NOLANE) sb_flush<C>(ytile, x, XC, tables, tile_lane, N);
}

static_assert(SB_LDS_WORDS(1, SB_C) * 4 <= 160 * 1024 && SB_LDS_WORDS(SB_WAVES, SB_C_ALT) * 4 <= 160 * 1024, "the tiles, the tables X and the run list lie in the CU's 160 KiB");

extern "C" uint64_t bqc_sbc_words(uint32_t n_lanes, uint32_t N) { return (uint64_t)n_lanes * 2 * BQC_SBC_MATE_WORDS(N); }

extern "C" void bqc_launch_sbc(const DevBatch& b, const DevRefs& refs, uint64_t* tables, uint32_t N, uint32_t Q, uint32_t MQ, uint32_t n_lanes, uint32_t n_cu, hipStream_t s)
{
    if (b.n_reads == 0) return;
    static const int alt = [] { const char* e = getenv("BQC_SBC_X"); return e && (e[0] == '1' || e[0] == '2') ? e[0] - '0' : 0; }(); // (the measured alternatives)
    static const hipError_t attr_0 = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sbc<1, SB_C>), hipFuncAttributeMaxDynamicSharedMemorySize, SB_LDS_WORDS(1, SB_C) * 4);
    static const hipError_t attr_1 = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sbc<1, SB_C_ALT>), hipFuncAttributeMaxDynamicSharedMemorySize, SB_LDS_WORDS(1, SB_C_ALT) * 4);
    static const hipError_t attr_2 = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sbc<SB_WAVES, SB_C_ALT>), hipFuncAttributeMaxDynamicSharedMemorySize, SB_LDS_WORDS(SB_WAVES, SB_C_ALT) * 4);
    (void)attr_0; (void)attr_1; (void)attr_2;
    const uint32_t grid = std::max(1u, std::min(n_cu, (b.n_reads + 255u) / 256u)); // about one workgroup per CU; a small batch gets fewer
    if (alt == 1) hipLaunchKernelGGL((k_sbc<1, SB_C_ALT>), dim3(grid), dim3(SB_THREADS), SB_LDS_WORDS(1, SB_C_ALT) * 4, s, b, refs, tables, N, Q, MQ, n_lanes);
    else if (alt == 2) hipLaunchKernelGGL((k_sbc<SB_WAVES, SB_C_ALT>), dim3(grid), dim3(SB_THREADS), SB_LDS_WORDS(SB_WAVES, SB_C_ALT) * 4, s, b, refs, tables, N, Q, MQ, n_lanes);
    else hipLaunchKernelGGL((k_sbc<1, SB_C>), dim3(grid), dim3(SB_THREADS), SB_LDS_WORDS(1, SB_C) * 4, s, b, refs, tables, N, Q, MQ, n_lanes);
}
