// k_mbc.hip — mismatches by cycle and base quality (--mismatch-by-cycle; the statistic: include/bamqc.h):
// A[lane][mate][cycle][q] counts the bases that were compared with the genome, M[lane][mate][cycle][q] those of them that differ.
// An optional module beside k_qcyc: its launch exists only when bqc_options.mismatch_by_cycle is set.
//
// Mapping.  About one workgroup per CU, MB_WAVES waves; a workgroup takes a contiguous share of the batch's processing order, MB_STEP
// reads at a time.  Thread t of a step fetches the columns of the step's read t, decides whether the read counts, and WALKS ITS CIGAR:
// every match-like operation (M, =, X) becomes a RUN [ia, ib) of stored positions, cut to the read, to the contig [0, len) and to the
// cycles below N, aligned at genome position posv + p.  The runs go to a list in LDS (slots handed out by an LDS counter; the order of
// the runs does not matter, every table is a sum).  A read of dozens of operations leaves dozens of runs: a thread that finds the list
// full keeps its walk where it is, the workgroup consumes the list and the threads go on filling it (rounds of a step) — no run is
// dropped, however many a step has.
// A wave takes ONE run per instruction: lane j owns the stored bases start + 4j .. + 3 (start = ia rounded down to 4), masked to the
// run; runs longer than 256 positions take further passes.  Qualities, nibbles and genome bytes each start anywhere, so each is one or
// two aligned dwords and a shift; only dwords that hold a byte of the run are touched (for the genome: a byte of [0, len)).  The loads
// of MB_U runs are requested together.
// Tables.  A is dense: [2 mates][MB_Q qualities][MB_C cycles] u32 in LDS (128 KiB), laid out and flushed as k_qcyc's tile (the 64 lanes
// of an LDS atomic hold 64 distinct cycles of one read).  M is sparse on real data — a fraction of a percent of A — and goes to device
// memory with one global atomic per mismatch: two 128 KiB tiles do not fit beside each other, and an input where every base mismatches
// is still counted exactly, only slowly.  What the tile does not hold (q >= MB_Q, cycles at or behind MB_C) goes to device memory too.
// The tile belongs to one read group at a time: it is flushed (non-zero bins only) when the read group changes and at the end.
#include <algorithm>
#include "kernels_common.h"
#include "mbc_walk.h" // the walk and the unaligned loads, shared with k_sbc.hip

#define MB_THREADS 1024
#define MB_WAVES (MB_THREADS / WAVE)
#define MB_Q 64
#define MB_C 256
#define MB_TILE (2 * MB_Q * MB_C)
#define MB_U 4                       // runs whose loads a wave requests together
#define MB_STEP 768                  // reads whose columns a workgroup fetches at a time, one per thread of its first MB_STEP
#define MB_RUNS 768                  // runs the list holds: a step of one-run reads is one round
#define MB_RW 8                      // words of a run
#define MB_WORDS (MB_TILE + MB_RW * MB_RUNS + 8)
#define MB_NOLANE 0xFFFFFFFFu
#define MB_QPAD 224                  // row of a table: Phred 0..222, padded

__device__ __forceinline__ uint32_t mb_swz(uint32_t c) { return (c & 3u) * 64u + (c >> 2); }

// What a lane holds of a run: its stored positions [lo, hi) (at most four; lo >= hi: none) and their bytes.
struct MbReq { uint32_t lo, hi, L, info; uintptr_t qa, sa, ga; uint64_t wq, ws, wg; };

// tables: those of the read group — [2 mates][A, M][N][MB_QPAD]
__device__ __forceinline__ void mb_count(const MbReq& q, uint32_t* tile, uint64_t* __restrict__ tables, uint32_t N)
{
    const uint32_t mate = (q.info >> 8) & 1u;
    const bool rev = (q.info >> 9) & 1u;
    uint64_t* A = tables + (uint64_t)mate * 2 * N * MB_QPAD;
    uint64_t* M = A + (uint64_t)N * MB_QPAD;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t p = q.lo + k;
        if (p >= q.hi) break;
        const uint32_t ql = mb_byte(q.wq, q.qa, k);
        const uint32_t sb = mb_byte(q.ws, q.sa, (p >> 1) - (q.lo >> 1));
        const uint32_t nib = (p & 1u) ? sb & 15u : sb >> 4;
        const uint32_t gc = mb_byte(q.wg, q.ga, k);
        const uint32_t c = rev ? q.L - 1u - p : p; // sequencing orientation
        if (!nib || (nib & (nib - 1u)) || gc > 3u || ql > 222u || c >= N) continue; // A, C, G, T against A, C, G, T
        if (ql < MB_Q && c < MB_C) atomicAdd(&tile[(mate * MB_Q + ql) * MB_C + mb_swz(c)], 1u);
        else gadd(A + (uint64_t)c * MB_QPAD + ql, 1);
        if ((uint32_t)__ffs((int)nib) - 1u != gc) gadd(M + (uint64_t)c * MB_QPAD + ql, 1);
    }
}

// tile -> table A of read group `lane`, and the tile back to zero
__device__ __forceinline__ void mb_flush(uint32_t* tile, uint64_t* __restrict__ tables, uint32_t lane, uint32_t N)
{
    block_sync();
    uint64_t* tl = tables + (uint64_t)lane * 4 * N * MB_QPAD;
    for (uint32_t t = threadIdx.x; t < MB_TILE; t += MB_THREADS) {
        const uint32_t v = tile[t];
        if (!v) continue;
        tile[t] = 0;
        const uint32_t mate = t / (MB_Q * MB_C), q = (t / MB_C) % MB_Q, pos = t % MB_C, c = (pos & 63u) * 4u + (pos >> 6);
        if (c < N) gadd(tl + ((uint64_t)mate * 2 * N + c) * MB_QPAD + q, v); // (a non-zero bin has c < N: said again where the address is made)
    }
    block_sync();
}

__global__ __launch_bounds__(MB_THREADS) void k_mbc(DevBatch b, DevRefs refs, uint64_t* __restrict__ tables, uint32_t N, uint32_t n_lanes)
{
    extern __shared__ uint32_t lds[];
    if (b.desc->fatal) return;
    uint32_t* tile = lds;
    uint32_t* s_qoff = lds + MB_TILE;
    uint32_t* s_soff = s_qoff + MB_RUNS;
    uint32_t* s_ia = s_soff + MB_RUNS;
    uint32_t* s_ib = s_ia + MB_RUNS;
    uint32_t* s_L = s_ib + MB_RUNS;
    uint32_t* s_galo = s_L + MB_RUNS;
    uint32_t* s_gahi = s_galo + MB_RUNS;
    uint32_t* s_info = s_gahi + MB_RUNS;
    uint32_t* s_ctl = s_info + MB_RUNS; // [0] slots asked for, [1] a thread found the list full, [2] lowest, [3] highest read group of the list, [4] the next one
    const uint32_t tid = threadIdx.x, wave = tid / WAVE, ln = lane_id();
    const uint32_t per = (uint32_t)(((uint64_t)b.n_reads + gridDim.x - 1) / gridDim.x);
    const uint64_t begin64 = (uint64_t)blockIdx.x * per;
    if (begin64 >= b.n_reads) return;
    const uint32_t begin = (uint32_t)begin64, end = (uint32_t)min((uint64_t)b.n_reads, begin64 + per);
    for (uint32_t t = tid; t < MB_TILE; t += MB_THREADS) tile[t] = 0;
    uint32_t tile_lane = MB_NOLANE;
    MbWalk w;
    for (uint32_t base = begin; base < end; base += MB_STEP) {
        mb_fetch(w, b, refs, tid < MB_STEP ? (uint64_t)base + tid : ~0ull, end, N, n_lanes);
        bool have = mb_next(w, b.cigar);
        for (;;) { // rounds of the step: one, unless its reads have more runs than the list holds
            if (tid == 0) { s_ctl[0] = 0; s_ctl[1] = 0; s_ctl[2] = MB_NOLANE; s_ctl[3] = 0; }
            block_sync();
            while (have) {
                const uint32_t slot = atomicAdd(&s_ctl[0], 1u);
                if (slot >= MB_RUNS) { s_ctl[1] = 1u; break; } // (full: this run waits for the next round)
                s_qoff[slot] = w.qoff; s_soff[slot] = w.soff; s_ia[slot] = w.ia; s_ib[slot] = w.ib; s_L[slot] = w.L;
                s_galo[slot] = (uint32_t)w.ga; s_gahi[slot] = (uint32_t)((uint64_t)w.ga >> 32); s_info[slot] = w.info;
                atomicMin(&s_ctl[2], w.info & 255u);
                atomicMax(&s_ctl[3], w.info & 255u);
                have = mb_next(w, b.cigar);
            }
            block_sync();
            const uint32_t n = min(s_ctl[0], (uint32_t)MB_RUNS);
            const bool more = s_ctl[1] != 0u;
            uint32_t cur = s_ctl[2];
            const uint32_t last = s_ctl[3];
            while (cur != MB_NOLANE) { // one pass per read group the list holds: one, unless the step spans a change of read group
                if (cur != tile_lane) {
                    if (tile_lane != MB_NOLANE) mb_flush(tile, tables, tile_lane, N);
                    tile_lane = cur;
                }
                uint64_t* tl = tables + (uint64_t)cur * 4 * N * MB_QPAD;
                // lane ln's part of pass `it` (256 stored positions a pass) of run e; runs behind n or of another read group: nothing
                auto request = [&](uint32_t e, uint32_t it) {
                    MbReq q;
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
                    q.qa = (uintptr_t)(b.qual + s_qoff[e]) + q.lo;
                    q.sa = (uintptr_t)(b.seq + s_soff[e]) + (q.lo >> 1);
                    q.ga = (uintptr_t)((uint64_t)s_gahi[e] << 32 | s_galo[e]) + q.lo;
                    q.wq = mb_load(q.qa, q.qa + (q.hi - 1u - q.lo));
                    q.ws = mb_load(q.sa, q.sa + (((q.hi - 1u) >> 1) - (q.lo >> 1)));
                    q.wg = mb_load(q.ga, q.ga + (q.hi - 1u - q.lo));
                    return q;
                };
                for (uint32_t e0 = wave * MB_U; e0 < n; e0 += MB_WAVES * MB_U) {
                    MbReq q[MB_U];
#pragma unroll
                    for (int u = 0; u < MB_U; ++u) q[u] = request(e0 + u, 0);
#pragma unroll
                    for (int u = 0; u < MB_U; ++u) mb_count(q[u], tile, tl, N);
#pragma unroll
                    for (int u = 0; u < MB_U; ++u) { // runs of more than 256 positions (ia rounded down included): further passes
                        if (e0 + u >= n) break;
                        const uint32_t span = s_ib[e0 + u] - (s_ia[e0 + u] & ~3u);
                        for (uint32_t it = 1; it < (span + 255u) / 256u; ++it) mb_count(request(e0 + u, it), tile, tl, N);
                    }
                }
                if (cur == last) break;
                block_sync();
                if (tid == 0) s_ctl[4] = MB_NOLANE;
                block_sync();
                if (tid < n && (s_info[tid] & 255u) > cur) atomicMin(&s_ctl[4], s_info[tid] & 255u);
                block_sync();
                cur = s_ctl[4];
            }
            block_sync(); // (the list is read to here)
            if (!more) break;
        }
        if (end - base <= MB_STEP) break; // (not left to the loop's test: base + MB_STEP may wrap)
    }
    if (tile_lane != MB_NOLANE) mb_flush(tile, tables, tile_lane, N);
}

extern "C" uint64_t bqc_mbc_words(uint32_t n_lanes, uint32_t N) { return (uint64_t)n_lanes * 2 * 2 * N * MB_QPAD; }

extern "C" void bqc_launch_mbc(const DevBatch& b, const DevRefs& refs, uint64_t* tables, uint32_t N, uint32_t n_lanes, uint32_t n_cu, hipStream_t s)
{
    if (b.n_reads == 0) return;
    static const hipError_t attr_once = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mbc), hipFuncAttributeMaxDynamicSharedMemorySize, MB_WORDS * 4);
    (void)attr_once;
    const uint32_t grid = std::max(1u, std::min(n_cu, (b.n_reads + 255u) / 256u)); // about one workgroup per CU; a small batch gets fewer
    hipLaunchKernelGGL(k_mbc, dim3(grid), dim3(MB_THREADS), MB_WORDS * 4, s, b, refs, tables, N, n_lanes);
}
