// k_adp.hip — adapter content by cycle (--adapter-by-cycle; the statistic: include/bamqc.h):
// F[lane][mate][slot][c] counts the examined reads whose FIRST occurrence of adapter `slot`, in sequencing orientation, starts at cycle
// c < N; E[lane][mate][min(L, N) - 1] counts the examined reads by length.  An optional module beside k_qcyc and k_mbc: its launch
// exists only when the context was made by bqc_create_ex with bqc_modules.adapter_by_cycle set.
//
// Mapping.  About one workgroup per CU, AD_WAVES waves; a workgroup takes a contiguous share of the batch's processing order, AD_STEP
// reads at a time, thread t of a step fetching the columns of the step's read t (and those of the next step before this one is searched).
// A lane OWNS 16 stored bases of a read and looks 15 ahead: the 31 bases are the 16 bytes behind the lane's first byte, taken as five
// aligned dwords and byte shifts (the bytes of a read start anywhere); only aligned dwords that hold a byte of the read are touched.
// A dword of eight nibbles becomes (ad_pack8, kernels_common.h) 16 bits of 2-bit codes and 8 bits of "is one of A, C, G, T"; what lies behind the read's last base —
// the pad nibble of an odd length, the next read's bytes, a dword that was not loaded — is cleared from the validity bits and so matches
// nothing.  Per adapter and offset 0..15 the test is one 64-bit shift, a mask, a compare and the validity test; the patterns are kernel
// arguments.  A reverse read is searched in STORED order for the reverse complement: its first hit in sequencing order is its LAST
// occurrence in stored order, at cycle L - p - m.
// The step's longest read decides how many lanes a read gets: w = the power of two at or above ceil(L / 16), at most 64, so a wave
// instruction holds 64 / w reads (150 bases: 16 lanes, four reads); reads of more than 1024 bases take further passes of the wave.
// Combining.  Hits are rare: a lane that finds one takes atomicMin on the LDS slot of (read of the step, adapter); the slots are reset
// every step.  Behind the step's barrier the thread of a read adds its first hits and its length.
// Tile.  [2 mates][9 rows][AD_C cycles] u32 in LDS (72 KiB); cycles at or behind AD_C go to the table in device memory with global atomics.
// u32 cannot wrap: a bin gets at most one increment per read.  The tile belongs to one read group at a time: it is flushed (non-zero
// bins only) when the read group changes and at the end.  Real data has ONE read length: the 64 threads of a wave would add to one LDS
// address, which serialises (profiles/r4_lds_atomic.txt) — equal (mate, length) pairs of a wave are counted by ballot and added once.
#include <algorithm>
#include "kernels_common.h"
#include "cigar_walk.h" // share_grid: the launch geometry of a kernel that shares the reads out

#define AD_THREADS 1024
#define AD_WAVES (AD_THREADS / WAVE)
#define AD_STEP AD_THREADS           // reads whose columns a workgroup fetches at a time, one per thread
#define AD_C 1024                    // cycles of the tile
#define AD_TILE (2 * BQC_ADP_ROWS * AD_C)
#define AD_WORDS (AD_TILE + 4 * AD_STEP + BQC_ADP_MAX * AD_STEP + 8)
#define AD_NOLANE 0xFFFFFFFFu
#define AD_NOHIT 0xFFFFFFFFu

// Chunk k of a read (stored bases 16 k .. 16 k + 30, the read has L > 16 k of them, its bytes start at seq + soff): every adapter's
// occurrences that START at one of the chunk's 16 owned bases, the one that comes first in sequencing order to the read's slot.
__device__ __forceinline__ void ad_search(const uint8_t* __restrict__ seq, uint32_t soff, uint32_t L, bool rev, uint32_t k, const AdpPatterns& P, uint32_t* hit /* the read's slot of adapter 0; stride AD_STEP */)
{
    const uintptr_t first = (uintptr_t)(seq + soff), end = first + ((uint64_t)L + 1) / 2, p = first + 8ull * k;
    const uint32_t sh = (uint32_t)p & 3u;
    const gmem_u32* a = (const gmem_u32*)(p & ~(uintptr_t)3); // (global, said so: through the integer the compiler sees a flat pointer)
    uint32_t d[5];
    d[0] = a[0]; // (holds byte p, a byte of the read)
#pragma unroll
    for (int i = 1; i < 5; ++i) d[i] = (uintptr_t)(a + i) < end ? a[i] : 0u;
    uint64_t codes = 0;
    uint32_t valid = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t c, v;
        ad_pack8(__builtin_amdgcn_alignbyte(d[i + 1], d[i], sh), c, v);
        codes |= (uint64_t)c << (16 * i);
        valid |= v << (8 * i);
    }
    const uint32_t s = 16u * k, left = L - s; // bases of the read from the chunk's first on
    if (left < 32u) valid &= (1u << left) - 1u;
    if (!valid) return;
#pragma unroll
    for (uint32_t ad = 0; ad < BQC_ADP_MAX; ++ad) {
        if (ad >= P.n) break;
        const uint32_t pat = rev ? P.rc[ad] : P.fwd[ad], cm = P.cmask[ad], vm = P.vmask[ad], m = P.len[ad];
        uint32_t hm = 0;
#pragma unroll
        for (uint32_t o = 0; o < 16; ++o) {
            const bool is = (((uint32_t)(codes >> (2 * o)) & cm) == pat) && (((valid >> o) & vm) == vm);
            hm |= (is ? 1u : 0u) << o;
        }
        if (hm) { // (all m bases valid: s + o + m <= L)
            const uint32_t pos = rev ? s + 31u - (uint32_t)__clz((int)hm) : s + (uint32_t)__ffs((int)hm) - 1u;
            atomicMin(&hit[ad * AD_STEP], rev ? L - pos - m : pos);
        }
    }
}

// tile -> table of read group `lane`, and the tile back to zero
__device__ __forceinline__ void ad_flush(uint32_t* tile, uint64_t* __restrict__ tab, uint32_t lane, uint32_t N)
{
    block_sync();
    uint64_t* tl = tab + (uint64_t)lane * 2 * BQC_ADP_ROWS * N;
    for (uint32_t t = threadIdx.x; t < AD_TILE; t += AD_THREADS) {
        const uint32_t v = tile[t];
        if (!v) continue;
        tile[t] = 0;
        gadd(tl + (uint64_t)(t / AD_C) * N + t % AD_C, v); // (t / AD_C = mate * 9 + row; a counted cycle is below N)
    }
    block_sync();
}

// Read i of the processing order: where its bases start, its length, mate and strand, and its read group (AD_NOLANE: not examined)
struct AdRead { uint32_t soff, L, info, lane; }; // info: mate | reverse << 1
__device__ __forceinline__ AdRead ad_fetch(const DevBatch& b, uint64_t i, uint32_t end, uint32_t n_lanes)
{
    AdRead o{0u, 0u, 0u, AD_NOLANE};
    if (i >= end) return o;
    const uint32_t r = b.order ? b.order[i] : (uint32_t)i;
    if (r >= b.n_reads) return o;
    const uint32_t f = b.flag[r], L = b.l_seq[r], g = b.lane[r];
    if ((f & 0x900u) || !(f & 0xC0u) || !L || g >= n_lanes) return o;
    o.soff = b.seq_off[r];
    o.L = L;
    o.info = ((f & 0x40u) ? 0u : 1u) | ((f >> 4) & 1u) << 1;
    o.lane = g;
    return o;
}

__global__ __launch_bounds__(AD_THREADS) void k_adp(DevBatch b, AdpPatterns P, uint64_t* __restrict__ tab, uint32_t N, uint32_t n_lanes, uint32_t per)
{
    extern __shared__ uint32_t lds[];
    if (b.desc->fatal) return;
    uint32_t* tile = lds;
    uint32_t* s_soff = lds + AD_TILE;
    uint32_t* s_L = s_soff + AD_STEP;
    uint32_t* s_info = s_L + AD_STEP;
    uint32_t* s_lane = s_info + AD_STEP;
    uint32_t* s_hit = s_lane + AD_STEP; // [adapter][read of the step]: the lowest cycle at which the adapter occurs, AD_NOHIT: nowhere
    uint32_t* s_mm = s_hit + BQC_ADP_MAX * AD_STEP; // [0] lowest, [1] highest read group of the step's examined reads, [2] the next one, [3] their longest read
    const uint32_t tid = threadIdx.x, wave = tid / WAVE, ln = lane_id();
    const uint64_t begin64 = (uint64_t)blockIdx.x * per;
    if (begin64 >= b.n_reads) return;
    const uint32_t begin = (uint32_t)begin64, end = (uint32_t)min((uint64_t)b.n_reads, begin64 + per);
    for (uint32_t t = tid; t < AD_TILE; t += AD_THREADS) tile[t] = 0;
    uint32_t tile_lane = AD_NOLANE;
    AdRead nx = ad_fetch(b, (uint64_t)begin + tid, end, n_lanes);
    for (uint32_t base = begin; base < end; base += AD_STEP) {
        const AdRead me = nx;
        if (end - base > AD_STEP) nx = ad_fetch(b, (uint64_t)base + AD_STEP + tid, end, n_lanes); // (in flight while this step is searched)
        s_soff[tid] = me.soff; s_L[tid] = me.L; s_info[tid] = me.info; s_lane[tid] = me.lane;
#pragma unroll
        for (uint32_t ad = 0; ad < BQC_ADP_MAX; ++ad) s_hit[ad * AD_STEP + tid] = AD_NOHIT;
        if (tid == 0) { s_mm[0] = AD_NOLANE; s_mm[1] = 0; s_mm[3] = 0; }
        block_sync();
        if (me.lane != AD_NOLANE) { atomicMin(&s_mm[0], me.lane); atomicMax(&s_mm[1], me.lane); atomicMax(&s_mm[3], me.L); }
        block_sync();
        uint32_t cur = s_mm[0];
        const uint32_t last = s_mm[1], longest = s_mm[3];
        const uint32_t nstep = min((uint32_t)AD_STEP, end - base);
        if (cur != AD_NOLANE) { // the search: every examined read of the step, whatever its read group (it does not touch the tile)
            const uint32_t chunks = (longest >> 4) + ((longest & 15u) ? 1u : 0u);
            const uint32_t lg = chunks >= 64u ? 6u : chunks <= 1u ? 0u : 32u - (uint32_t)__clz((int)(chunks - 1u)); // lanes per read: 1 << lg
            const uint32_t rp = 64u >> lg, sub = ln >> lg, j = ln & ((1u << lg) - 1u);
            for (uint32_t g = wave * rp + sub; g < nstep; g += AD_WAVES * rp) {
                if (s_lane[g] == AD_NOLANE) continue;
                const uint32_t L = s_L[g], soff = s_soff[g], nch = (L >> 4) + ((L & 15u) ? 1u : 0u);
                const bool rev = (s_info[g] >> 1) & 1u;
                for (uint32_t k = j; k < nch; k += 64u) ad_search(b.seq, soff, L, rev, k, P, s_hit + g); // (1 << lg < 64: nch <= 1 << lg, one pass)
            }
        }
        block_sync();
        while (cur != AD_NOLANE) { // one round per read group the step holds: one, unless the step spans a change of read group
            if (cur != tile_lane) {
                if (tile_lane != AD_NOLANE) ad_flush(tile, tab, tile_lane, N);
                tile_lane = cur;
            }
            uint64_t* tl = tab + (uint64_t)cur * 2 * BQC_ADP_ROWS * N;
            const bool mine = me.lane == cur;
            const uint32_t mate = me.info & 1u, row0 = mate * BQC_ADP_ROWS;
            if (mine) {
#pragma unroll
                for (uint32_t ad = 0; ad < BQC_ADP_MAX; ++ad) {
                    if (ad >= P.n) break;
                    const uint32_t h = s_hit[ad * AD_STEP + tid];
                    if (h >= N) continue; // (no hit, or a first hit at or behind the capacity)
                    if (h < AD_C) atomicAdd(&tile[(row0 + ad) * AD_C + h], 1u);
                    else gadd(tl + (uint64_t)(row0 + ad) * N + h, 1);
                }
            }
            // the reads by length: equal (mate, length) pairs of the wave are added once
            const uint32_t e = min(me.L, N) - 1u, key = e | mate << 31; // (N < 2^30)
            uint64_t m = __ballot(mine);
            while (m) {
                const int leader = __ffsll((unsigned long long)m) - 1;
                const uint32_t k0 = __builtin_amdgcn_readlane(key, leader);
                const uint64_t sm = __ballot(mine && key == k0);
                if ((int)ln == leader) {
                    const uint32_t cnt = (uint32_t)__popcll((unsigned long long)sm);
                    if (e < AD_C) atomicAdd(&tile[(row0 + BQC_ADP_MAX) * AD_C + e], cnt);
                    else gadd(tl + (uint64_t)(row0 + BQC_ADP_MAX) * N + e, cnt);
                }
                m &= ~sm;
            }
            if (cur == last) break;
            block_sync();
            if (tid == 0) s_mm[2] = AD_NOLANE;
            block_sync();
            if (me.lane != AD_NOLANE && me.lane > cur) atomicMin(&s_mm[2], me.lane);
            block_sync();
            cur = s_mm[2];
        }
        block_sync(); // (the step's tables are read to here)
        if (end - base <= AD_STEP) break; // (not left to the loop's test: base + AD_STEP may wrap)
    }
    if (tile_lane != AD_NOLANE) ad_flush(tile, tab, tile_lane, N);
}

extern "C" uint64_t bqc_adp_words(uint32_t n_lanes, uint32_t N) { return (uint64_t)n_lanes * 2 * BQC_ADP_ROWS * N; }

// workgroups: about one per CU, a small batch gets fewer; each takes `per` consecutive reads of the processing order
extern "C" void bqc_launch_adp(const DevBatch& b, const AdpPatterns& P, uint64_t* tab, uint32_t N, uint32_t n_lanes, uint32_t n_cu, hipStream_t s)
{
    if (b.n_reads == 0) return;
    static const hipError_t attr_once = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_adp), hipFuncAttributeMaxDynamicSharedMemorySize, AD_WORDS * 4);
    (void)attr_once;
    uint32_t per;
    const uint32_t g = share_grid(b.n_reads, n_cu, &per);
    hipLaunchKernelGGL(k_adp, dim3(g), dim3(AD_THREADS), AD_WORDS * 4, s, b, P, tab, N, n_lanes, per);
}
