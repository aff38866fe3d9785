// k_qcyc.hip — per-cycle base quality histograms (--qual-by-cycle): H[lane][mate][cycle][q], one increment
// per counted base.  An optional module beside the sketch: its launch exists only when bqc_options.qual_by_cycle is set.
//
// Mapping.  About one workgroup per CU, QC_WAVES waves.  A workgroup belongs to a ROW of QC_C cycles (row r: cycles 256 r .. 256 r + 255;
// the last row also takes whatever lies behind it) and takes a contiguous share of the batch's processing order; of every read it looks
// at the bytes of its row's cycles only.  A batch of short reads has one row; with reads of 256 bases and more there are as many as the
// capacity N and the longest read ask for, row 0 with workgroups in proportion to all reads, the others to the long ones.
// A wave takes ONE read per instruction: lane j owns the stored quality bytes 4j .. 4j+3 of the read's part in the row (two aligned
// dword loads and a byte shift, as the bytes of a read start anywhere), so the 64 lanes of an LDS atomic hold 64 DISTINCT cycles of one
// read — never the same (cycle, quality) bin twice, which is what serialises an LDS atomic and what binned qualities would make the
// common case if lanes held the same cycle of different reads.  The loads of QC_U reads are requested together, and those of the next
// QC_U before the first QC_U are counted: the kernel lives on loads in flight, not on arithmetic.
// Tile.  [2 mates][QC_Q qualities][QC_C cycles] u32 in LDS (128 KiB): cycle t of the row sits at (t & 3) * 64 + (t >> 2), so the k-th
// bytes of consecutive lanes (cycles 4 apart, ascending or — reverse reads — descending) fall on consecutive banks; the row stride
// (256 dwords) is a multiple of the 32 banks, so this holds whatever q is.  u32 counters cannot wrap: a bin gets at most one
// increment per read and a batch has fewer than 2^32 reads.  What the tile does not hold (q >= QC_Q; cycles behind the last row, which
// exist only when the launcher's longest read was an underestimate) goes to the table in device memory with global atomics.
// The tile belongs to one read group at a time: it is flushed (non-zero bins only) when the read group changes and at the end.
#include <algorithm>
#include "kernels_common.h"

#define QC_THREADS 1024
#define QC_WAVES (QC_THREADS / WAVE)
#define QC_Q 64
#define QC_C 256
#define QC_TILE (2 * QC_Q * QC_C)
#define QC_U 6                       // reads whose loads a wave requests together (two such groups are in flight)
// reads whose columns a workgroup fetches at a time, one per thread of its first QC_STEP: a whole number of groups per wave (960)
#define QC_STEP (QC_WAVES * QC_U * (QC_THREADS / (QC_WAVES * QC_U)))
#define QC_WORDS (QC_TILE + 3 * QC_STEP + 4)
#define QC_NOLANE 0xFFFFFFFFu
#define QC_QPAD 224                  // row of the table: Phred 0..222, padded
#define QC_CNT_MASK 0x3FFFFFFFu      // info word of a read: counted bytes (those of the row's cycles) | mate << 30 | reverse << 31

__device__ __forceinline__ uint32_t qc_swz(uint32_t c) { return (c & 3u) * 64u + (c >> 2); }

// the four bytes qual[at + off .. + 4) as one dword (byte 0 lowest); bytes at or behind `cnt` are undefined.  Only aligned dwords that
// hold at least one byte of the read are touched: such a dword lies in the page of that byte.
__device__ __forceinline__ uint32_t qc_load4(const uint8_t* __restrict__ qual, uint32_t at, uint32_t off, uint32_t cnt)
{
    const uintptr_t p = (uintptr_t)(qual + (uint64_t)at + off);
    const uint32_t sh = (uint32_t)p & 3u;
    const gmem_u32* a = (const gmem_u32*)(p & ~(uintptr_t)3); // (global, said so: through the integer the compiler sees a flat pointer)
    const uint32_t lo = a[0];
    uint32_t hi = 0;
    if (sh && off + 4u - sh < cnt) hi = a[1];
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
}

// hl: the read group's table, moved on to the row's first cycle
__device__ __forceinline__ void qc_count4(uint32_t v, uint32_t off, uint32_t info, uint32_t* tile, uint64_t* __restrict__ hl, uint32_t N)
{
    const uint32_t cnt = info & QC_CNT_MASK, mate = (info >> 30) & 1u;
    const bool rev = info >> 31;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t i = off + k;
        if (i >= cnt) break;
        const uint32_t q = (v >> (8 * k)) & 255u;
        const uint32_t c = rev ? cnt - 1u - i : i; // sequencing orientation, relative to the row's first cycle; row start + c < N
        if (q < QC_Q && c < QC_C) atomicAdd(&tile[(mate * QC_Q + q) * QC_C + qc_swz(c)], 1u);
        else if (q <= 222u) gadd(hl + ((uint64_t)mate * N + c) * QC_QPAD + q, 1);
    }
}

// tile -> table of read group `lane`, and the tile back to zero
__device__ __forceinline__ void qc_flush(uint32_t* tile, uint64_t* __restrict__ hist, uint32_t lane, uint32_t N, uint32_t c_base)
{
    block_sync();
    uint64_t* hl = hist + ((uint64_t)lane * 2 * N + c_base) * QC_QPAD;
    for (uint32_t t = threadIdx.x; t < QC_TILE; t += QC_THREADS) {
        const uint32_t v = tile[t];
        if (!v) continue;
        tile[t] = 0;
        const uint32_t mate = t / (QC_Q * QC_C), q = (t / QC_C) % QC_Q, pos = t % QC_C, c = (pos & 63u) * 4u + (pos >> 6);
        gadd(hl + ((uint64_t)mate * N + c) * QC_QPAD + q, v);
    }
    block_sync();
}

// Read i of the processing order in the row of cycles [c_base, c_base + QC_C) (the last row: [c_base, N)): where its bytes of those
// cycles start, how many there are, mate and strand, and its read group (QC_NOLANE: the read does not count, or ends before the row).
struct QcRead { uint32_t qbeg, info, lane; };
__device__ __forceinline__ QcRead qc_fetch(const DevBatch& b, uint64_t i, uint32_t end, uint32_t N, uint32_t n_lanes, uint32_t c_base, bool last_row)
{
    QcRead o{0u, 0u, QC_NOLANE};
    if (i >= end) return o;
    const uint32_t r = b.order ? b.order[i] : (uint32_t)i;
    if (r >= b.n_reads) return o;
    const uint32_t f = b.flag[r], L = b.l_seq[r], g = b.lane[r];
    if ((f & 0x900u) || !(f & 0xC0u) || (f & BQC_FLAG_NO_QUAL) || !L || g >= n_lanes) return o;
    const uint32_t cnt = min(L, N), rev = (f >> 4) & 1u; // cycles counted of the read: [0, cnt)
    if (cnt <= c_base) return o;
    const uint32_t c_hi = last_row ? cnt : min(cnt, c_base + QC_C);
    // cycle c is stored byte c of a forward read and byte L - 1 - c of a reverse one: the row's cycles [c_base, c_hi) are the bytes
    // [c_base, c_hi), or [L - c_hi, L - c_base) — counted from there, byte i is cycle c_base + i, or c_hi - 1 - i
    o.qbeg = b.qual_off[r] + (rev ? L - c_hi : c_base);
    o.info = (c_hi - c_base) | ((f & 0x40u) ? 0u : 1u << 30) | rev << 31;
    o.lane = g;
    return o;
}

// g0 workgroups for row 0, g1 for each further row (blockIdx.x = g0 + (row - 1) * g1 + x)
__global__ __launch_bounds__(QC_THREADS) void k_qcyc(DevBatch b, uint64_t* __restrict__ hist, uint32_t N, uint32_t n_lanes, uint32_t g0, uint32_t g1, uint32_t rows)
{
    extern __shared__ uint32_t lds[];
    if (b.desc->fatal) return;
    uint32_t* tile = lds;
    uint32_t* s_qbeg = lds + QC_TILE;
    uint32_t* s_info = s_qbeg + QC_STEP;
    uint32_t* s_lane = s_info + QC_STEP;
    uint32_t* s_mm = s_lane + QC_STEP; // [0] lowest, [1] highest read group of the step's counted reads, [2] the next one
    const uint32_t tid = threadIdx.x, wave = tid / WAVE, ln = lane_id();
    const uint32_t row = blockIdx.x < g0 ? 0u : 1u + (blockIdx.x - g0) / g1, x = blockIdx.x < g0 ? blockIdx.x : (blockIdx.x - g0) % g1, gx = row ? g1 : g0;
    const uint32_t c_base = row * QC_C;
    const bool last_row = row + 1 == rows;
    const uint32_t per = (uint32_t)(((uint64_t)b.n_reads + gx - 1) / gx);
    const uint64_t begin64 = (uint64_t)x * per;
    if (begin64 >= b.n_reads || c_base >= N) return;
    const uint32_t begin = (uint32_t)begin64, end = (uint32_t)min((uint64_t)b.n_reads, begin64 + per);
    for (uint32_t t = tid; t < QC_TILE; t += QC_THREADS) tile[t] = 0;
    uint32_t tile_lane = QC_NOLANE;
    const uint64_t none = ~0ull; // (threads behind QC_STEP fetch no read)
    QcRead nx = qc_fetch(b, tid < QC_STEP ? (uint64_t)begin + tid : none, end, N, n_lanes, c_base, last_row);
    for (uint32_t base = begin; base < end; base += QC_STEP) {
        const uint32_t my_lane = nx.lane, qbeg = nx.qbeg, info = nx.info;
        if (end - base > QC_STEP) nx = qc_fetch(b, tid < QC_STEP ? (uint64_t)base + QC_STEP + tid : none, end, N, n_lanes, c_base, last_row); // (in flight while this step is counted)
        if (tid < QC_STEP) { s_qbeg[tid] = qbeg; s_info[tid] = info; s_lane[tid] = my_lane; }
        if (tid == 0) { s_mm[0] = QC_NOLANE; s_mm[1] = 0; }
        block_sync();
        if (my_lane != QC_NOLANE) { atomicMin(&s_mm[0], my_lane); atomicMax(&s_mm[1], my_lane); }
        block_sync();
        uint32_t cur = s_mm[0];
        const uint32_t last = s_mm[1];
        const uint32_t nstep = min((uint32_t)QC_STEP, end - base);
        while (cur != QC_NOLANE) { // one round per read group the step holds: one, unless the step spans a change of read group
            if (cur != tile_lane) {
                if (tile_lane != QC_NOLANE) qc_flush(tile, hist, tile_lane, N, c_base);
                tile_lane = cur;
            }
            uint64_t* hl = hist + ((uint64_t)cur * 2 * N + c_base) * QC_QPAD;
            // the reads g .. g + QC_U - 1 of the step (g + u < QC_STEP; reads behind nstep, of another read group or outside the row have info 0)
            auto request = [&](uint32_t g, uint32_t (&inf)[QC_U], uint32_t (&v)[QC_U]) {
#pragma unroll
                for (int u = 0; u < QC_U; ++u) {
                    inf[u] = s_lane[g + u] == cur ? s_info[g + u] : 0u;
                    v[u] = 0;
                    if (4u * ln < (inf[u] & QC_CNT_MASK)) v[u] = qc_load4(b.qual, s_qbeg[g + u], 4u * ln, inf[u] & QC_CNT_MASK);
                }
            };
            auto count = [&](uint32_t g, const uint32_t (&inf)[QC_U], const uint32_t (&v)[QC_U]) {
#pragma unroll
                for (int u = 0; u < QC_U; ++u) qc_count4(v[u], 4u * ln, inf[u], tile, hl, N);
#pragma unroll
                for (int u = 0; u < QC_U; ++u) { // more than 256 bytes: only in the last row, behind its tile
                    const uint32_t cnt = inf[u] & QC_CNT_MASK;
                    for (uint32_t off = 256u + 4u * ln; off < cnt; off += 256u)
                        qc_count4(qc_load4(b.qual, s_qbeg[g + u], off, cnt), off, inf[u], tile, hl, N);
                }
            };
            const uint32_t stride = QC_WAVES * QC_U;
            uint32_t infA[QC_U], vA[QC_U], infB[QC_U], vB[QC_U];
            uint32_t g = wave * QC_U;
            if (g < nstep) request(g, infA, vA);
            while (g < nstep) { // two groups in flight: the next one's loads are requested before this one is counted
                const uint32_t g1n = g + stride, g2n = g1n + stride;
                if (g1n < nstep) request(g1n, infB, vB);
                count(g, infA, vA);
                if (g2n < nstep) request(g2n, infA, vA);
                if (g1n < nstep) count(g1n, infB, vB);
                g = g2n;
            }
            if (cur == last) break;
            block_sync();
            if (tid == 0) s_mm[2] = QC_NOLANE;
            block_sync();
            if (my_lane != QC_NOLANE && my_lane > cur) atomicMin(&s_mm[2], my_lane);
            block_sync();
            cur = s_mm[2];
        }
        block_sync(); // (the step's tables are read to here)
        if (end - base <= QC_STEP) break; // (not left to the loop's test: base + QC_STEP may wrap)
    }
    if (tile_lane != QC_NOLANE) qc_flush(tile, hist, tile_lane, N, c_base);
}

extern "C" uint64_t bqc_qcyc_words(uint32_t n_lanes, uint32_t N) { return (uint64_t)n_lanes * 2 * N * QC_QPAD; }

// n_long / longest: the batch's reads of QC_C bases and more (an upper bound will do: what lies behind the last row is still counted)
extern "C" void bqc_launch_qcyc(const DevBatch& b, uint64_t* hist, uint32_t N, uint32_t n_lanes, uint32_t n_cu, uint32_t n_long, uint32_t longest, hipStream_t s)
{
    if (b.n_reads == 0) return;
    static const hipError_t attr_once = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_qcyc), hipFuncAttributeMaxDynamicSharedMemorySize, QC_WORDS * 4);
    (void)attr_once;
    const uint32_t top = std::min(N, n_long ? std::max(longest, (uint32_t)QC_C) : (uint32_t)QC_C - 1u);
    const uint32_t rows = std::min((top + QC_C - 1) / QC_C, 64u); // (64 rows: cycles behind 16 384 go out with global atomics)
    // workgroups: about one per CU in all; row 0 in proportion to all reads, every further row to the long ones; a small batch gets fewer
    const uint64_t w0 = b.n_reads, w1 = n_long, wsum = w0 + (uint64_t)(rows - 1) * w1;
    uint32_t g1 = rows > 1 ? (uint32_t)std::max<uint64_t>(1, n_cu * w1 / wsum) : 1u;
    uint32_t g0 = (uint32_t)std::max<uint64_t>(1, n_cu * w0 / wsum);
    g0 = std::max(1u, std::min(g0, (uint32_t)((w0 + 255) / 256)));
    g1 = std::max(1u, std::min(g1, (uint32_t)((w1 + 255) / 256)));
    hipLaunchKernelGGL(k_qcyc, dim3(g0 + (rows - 1) * g1), dim3(QC_THREADS), QC_WORDS * 4, s, b, hist, N, n_lanes, g0, g1, rows);
}
