// k_ibc.hip — indels by cycle and by length (--indel-by-cycle; the statistic: include/bamqc.h): per read group and
// mate E[min(L, N) - 1] counts the examined reads, IC[c] / DC[c] the insertion / deletion events at cycle c < N, IL / DL the events by
// length (64 bins, the last one open).  An optional module beside k_qcyc, k_mbc, k_adp and k_gcb_reads: its launch exists only when
// bqc_enable_indel_by_cycle has been called.  The genome is not read.
//
// Mapping.  The walk frame of cigar_walk.h: about one workgroup per CU, IB_WAVES waves; a workgroup takes a contiguous share of the
// batch's processing order, IB_STEP reads at a time, thread t of a step fetching the columns of the step's read t (and those of the
// next step before this one is walked).
// Short CIGARs.  A read of at most T operations (T = IB_T = 8 unless the launch says otherwise) is walked by its own thread: its first
// IB_T words are loaded together into registers, the walk is 64-bit per thread.
// Long CIGARs.  A read of more operations goes onto a list in LDS; behind the barrier the workgroup's waves take one listed read each at
// a time, 64 operations a pass (CigWalk without the genome's side: the exact stored index j of every operation).  Once the carry has
// reached L no later operation can be an event (both kinds need j < L), and the read is left.
// Tile.  [2 mates][3 rows][IB_C cycles] + [2 mates][2][64] u32 in LDS (25 KiB); cycles at or behind IB_C go to the table in device memory
// with gadd.  The tile belongs to one read group at a time: it is flushed (non-zero bins only) when the read group changes and at the
// end.  u32 cannot wrap between flushes: a CIGAR operation adds at most 1 to one cycle bin and 1 to one length bin, a read 1 to one E
// bin, so no bin receives more than the operations (or reads) of the workgroup's share — and the pre-pass refuses a batch whose CIGAR
// words do not fit 32-bit offsets (error key 3, desc->fatal: the kernel returns at once).
// Hot bins.  Real data has ONE read length, and nearly every indel has length 1: 64 lanes adding to one LDS address serialise
// (profiles/r4_lds_atomic.txt) — equal (mate, bin) pairs of a wave are counted by ballot and added once, for E, IL and DL.  IC and DC
// take plain LDS atomics: an event's cycle is spread over the read.
#include "cigar_walk.h"

#define IB_THREADS 1024
#define IB_WAVES (IB_THREADS / WAVE)
#define IB_STEP IB_THREADS           // reads whose columns a workgroup fetches at a time, one per thread
#define IB_T 8                       // operations up to which a read is walked by its own thread
#define IB_C 1024                    // cycles of the tile
#define IB_TILE_C (2 * BQC_IBC_ROWS * IB_C)
#define IB_TILE (IB_TILE_C + 2 * 2 * BQC_IBC_K)
#define IB_NOLANE 0xFFFFFFFFu

// Read i of the processing order: its length, CIGAR, mate and strand, and its read group (IB_NOLANE: not examined)
struct IbRead { uint32_t L, nc, coff, info, lane; }; // info: mate | reverse << 1
__device__ __forceinline__ IbRead ib_fetch(const DevBatch& b, uint64_t i, uint32_t end, uint32_t n_lanes)
{
    IbRead o{0u, 0u, 0u, 0u, IB_NOLANE};
    const uint32_t r = batch_read(b, i, end);
    if (r == WALK_NONE) return o;
    const uint32_t f = b.flag[r], L = b.l_seq[r], g = b.lane[r], nc = b.n_cigar[r];
    if ((f & 0x904u) || !(f & 0xC0u) || !L || !nc || g >= n_lanes) return o;
    o.L = L;
    o.nc = nc;
    o.coff = b.cigar_off[r];
    o.info = ((f & 0x40u) ? 0u : 1u) | ((f >> 4) & 1u) << 1;
    o.lane = g;
    return o;
}

// tile -> tables of read group `lane`, and the tile back to zero
__device__ __forceinline__ void ib_flush(uint32_t* tile, uint64_t* __restrict__ tab, uint32_t lane, uint32_t N)
{
    block_sync();
    const uint64_t mw = BQC_IBC_MATE_WORDS(N);
    uint64_t* tl = tab + (uint64_t)lane * 2 * mw;
    for (uint32_t t = threadIdx.x; t < IB_TILE; t += IB_THREADS) {
        const uint32_t v = tile[t];
        if (!v) continue;
        tile[t] = 0;
        if (t < IB_TILE_C) {
            const uint32_t mr = t / IB_C; // mate * 3 + row; a counted cycle is below N
            gadd(tl + (uint64_t)(mr / BQC_IBC_ROWS) * mw + (uint64_t)(mr % BQC_IBC_ROWS) * N + t % IB_C, v);
        } else {
            const uint32_t u = t - IB_TILE_C; // mate * 128 + kind * 64 + bin
            gadd(tl + (uint64_t)(u / (2 * BQC_IBC_K)) * mw + (uint64_t)BQC_IBC_ROWS * N + u % (2 * BQC_IBC_K), v);
        }
    }
    block_sync();
}

// One CIGAR operation at stored index j of a read of L bases: is it an event, of which kind (0 insertion, 1 deletion), at which cycle
__device__ __forceinline__ bool ib_event(uint32_t op, uint32_t n, uint64_t j, uint32_t L, bool rev, uint32_t N, uint32_t& kind, uint32_t& c)
{
    bool ev = false;
    kind = 0; c = 0;
    if (op == 1u) {
        ev = n >= 1u && j + n <= (uint64_t)L;
        c = rev ? L - (uint32_t)j - n : (uint32_t)j; // (an event: j + n <= L)
    } else if (op == 2u) {
        ev = n >= 1u && j > 0 && j < (uint64_t)L;
        kind = 1u;
        c = rev ? L - 1u - (uint32_t)j : (uint32_t)j - 1u;
    }
    return ev && c < N;
}

// An event of every lane with `ev` (called by whole waves): its cycle bin by an atomic of its own, its length bin once per distinct
// (mate, kind, bin) of the wave.  tm: the (lane, mate)'s words in device memory.
__device__ __forceinline__ void ib_count(bool ev, uint32_t mate, uint32_t kind, uint32_t c, uint32_t n, uint32_t* tile, uint64_t* tm, uint32_t N)
{
    uint64_t m = __ballot(ev);
    if (!m) return;
    if (ev) {
        if (c < IB_C) atomicAdd(&tile[(mate * BQC_IBC_ROWS + 1u + kind) * IB_C + c], 1u);
        else gadd(tm + (uint64_t)(1u + kind) * N + c, 1);
    }
    const uint32_t key = mate * (2 * BQC_IBC_K) + kind * BQC_IBC_K + min(n, (uint32_t)BQC_IBC_K) - 1u; // (ev: n >= 1)
    const uint32_t ln = lane_id();
    while (m) {
        const int leader = __ffsll((unsigned long long)m) - 1;
        const uint32_t k0 = __builtin_amdgcn_readlane(key, leader);
        const uint64_t sm = __ballot(ev && key == k0);
        if ((int)ln == leader) atomicAdd(&tile[IB_TILE_C + k0], (uint32_t)__popcll((unsigned long long)sm));
        m &= ~sm;
    }
}

__global__ __launch_bounds__(IB_THREADS) void k_ibc(DevBatch b, uint64_t* __restrict__ tab, uint32_t N, uint32_t n_lanes, uint32_t per, uint32_t t_max)
{
    __shared__ uint32_t tile[IB_TILE];
    __shared__ uint32_t s_list[IB_STEP];  // the threads whose reads take the wave path, this round
    __shared__ uint32_t s_L[IB_STEP], s_nc[IB_STEP], s_coff[IB_STEP], s_info[IB_STEP]; // their reads, by thread
    __shared__ uint32_t s_mm[4];          // [0] lowest, [1] highest read group of the step's examined reads, [2] the next one, [3] listed reads
    if (b.desc->fatal) return;
    const uint32_t tid = threadIdx.x, wave = tid / WAVE, ln = lane_id();
    uint32_t begin, end;
    if (!wg_share(b.n_reads, per, begin, end)) return;
    const gmem_u32* cg = (const gmem_u32*)(uintptr_t)b.cigar;
    const uint64_t mw = BQC_IBC_MATE_WORDS(N);
    for (uint32_t t = tid; t < IB_TILE; t += IB_THREADS) tile[t] = 0;
    uint32_t tile_lane = IB_NOLANE;
    IbRead nx = ib_fetch(b, (uint64_t)begin + tid, end, n_lanes);
    for (uint32_t base = begin; base < end; base += IB_STEP) {
        const IbRead me = nx;
        const bool thr = me.lane != IB_NOLANE && me.nc <= t_max; // walked by this thread
        uint32_t w[IB_T];
#pragma unroll
        for (uint32_t k = 0; k < IB_T; ++k) w[k] = thr && k < me.nc ? cg[(uint64_t)me.coff + k] : 0u; // (0: M of no bases, which does nothing)
        if (!last_step(base, end, IB_STEP)) nx = ib_fetch(b, (uint64_t)base + IB_STEP + tid, end, n_lanes); // (in flight while this step is walked)
        if (tid == 0) { s_mm[0] = IB_NOLANE; s_mm[1] = 0; s_mm[3] = 0; }
        block_sync();
        if (me.lane != IB_NOLANE) { atomicMin(&s_mm[0], me.lane); atomicMax(&s_mm[1], me.lane); }
        block_sync();
        uint32_t cur = s_mm[0];
        const uint32_t last = s_mm[1];
        const uint32_t mate = me.info & 1u;
        const bool rev = (me.info >> 1) & 1u;
        while (cur != IB_NOLANE) { // one round per read group the step holds: one, unless the step spans a change of read group
            if (cur != tile_lane) {
                if (tile_lane != IB_NOLANE) ib_flush(tile, tab, tile_lane, N);
                tile_lane = cur;
            }
            uint64_t* tl = tab + (uint64_t)cur * 2 * mw;
            const bool mine = me.lane == cur;
            // the reads by length: equal (mate, length) pairs of the wave are added once
            {
                const uint32_t e = min(me.L, N) - 1u, key = e | mate << 31; // (N < 2^30)
                uint64_t m = __ballot(mine);
                while (m) {
                    const int leader = __ffsll((unsigned long long)m) - 1;
                    const uint32_t k0 = __builtin_amdgcn_readlane(key, leader);
                    const uint64_t sm = __ballot(mine && key == k0);
                    if ((int)ln == leader) {
                        const uint32_t cnt = (uint32_t)__popcll((unsigned long long)sm);
                        if (e < IB_C) atomicAdd(&tile[mate * BQC_IBC_ROWS * IB_C + e], cnt);
                        else gadd(tl + (uint64_t)mate * mw + e, cnt);
                    }
                    m &= ~sm;
                }
            }
            // the thread path
            const bool walk = mine && thr;
            if (__ballot(walk)) {
                uint64_t j = 0;
                uint64_t* tm = tl + (uint64_t)mate * mw;
                auto step = [&](uint32_t wd) {
                    const uint32_t op = wd & 15u, n = wd >> 4;
                    uint32_t kind = 0, c = 0;
                    const bool ev = walk && ib_event(op, n, j, me.L, rev, N, kind, c);
                    j += cig_qlen(op, n);
                    ib_count(ev, mate, kind, c, n, tile, tm, N);
                };
#pragma unroll
                for (uint32_t k = 0; k < IB_T; ++k) step(w[k]);
                if (t_max > IB_T) { // (a launch that sends longer CIGARs down this path: tools/ibc_time.py's comparison)
                    uint32_t kmax = walk ? me.nc : 0u;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o));
                    for (uint32_t k = IB_T; k < kmax; ++k) step(walk && k < me.nc ? cg[(uint64_t)me.coff + k] : 0u);
                }
            }
            // the wave path: the round's long reads onto the list, then a wave per listed read
            if (mine && !thr) {
                s_list[atomicAdd(&s_mm[3], 1u)] = tid;
                s_L[tid] = me.L; s_nc[tid] = me.nc; s_coff[tid] = me.coff; s_info[tid] = me.info;
            }
            block_sync();
            const uint32_t listed = s_mm[3];
            for (uint32_t e = wave; e < listed; e += IB_WAVES) {
                const uint32_t t = s_list[e];
                const uint32_t L = __builtin_amdgcn_readfirstlane(s_L[t]), nc = __builtin_amdgcn_readfirstlane(s_nc[t]);
                const uint32_t coff = __builtin_amdgcn_readfirstlane(s_coff[t]), info = __builtin_amdgcn_readfirstlane(s_info[t]);
                const uint32_t mt = info & 1u;
                const bool rv = (info >> 1) & 1u;
                uint64_t* tm = tl + (uint64_t)mt * mw;
                CigWalk<false> cw;
                cw.start(cg, coff, nc, L);
                for (uint32_t p = 0; p < nc; p += WAVE) {
                    uint32_t op, n, kind, c; uint64_t jj; int64_t gg;
                    cw.pass(p, op, n, jj, gg);
                    const bool ev = ib_event(op, n, jj, L, rv, N, kind, c);
                    ib_count(ev, mt, kind, c, n, tile, tm, N);
                    if (!cw.advance()) break; // (both kinds of event need j < L)
                }
            }
            if (cur == last) break;
            block_sync();
            if (tid == 0) { s_mm[2] = IB_NOLANE; s_mm[3] = 0; }
            block_sync();
            if (me.lane != IB_NOLANE && me.lane > cur) atomicMin(&s_mm[2], me.lane);
            block_sync();
            cur = s_mm[2];
        }
        block_sync(); // (the step's list is read to here)
        if (last_step(base, end, IB_STEP)) break;
    }
    if (tile_lane != IB_NOLANE) ib_flush(tile, tab, tile_lane, N);
}

extern "C" uint64_t bqc_ibc_words(uint32_t n_lanes, uint32_t N) { return (uint64_t)n_lanes * 2 * BQC_IBC_MATE_WORDS(N); }

// BQC_IBC_T=n (a measuring switch): reads of up to n operations take the thread path instead of IB_T.
extern "C" void bqc_launch_ibc(const DevBatch& b, uint64_t* tab, uint32_t N, uint32_t n_lanes, uint32_t n_cu, hipStream_t s)
{
    if (b.n_reads == 0) return;
    static const uint32_t t_max = env_uint("BQC_IBC_T", IB_T, 65535, IB_T);
    uint32_t per;
    const uint32_t g = share_grid(b.n_reads, n_cu, &per);
    hipLaunchKernelGGL(k_ibc, dim3(g), dim3(IB_THREADS), 0, s, b, tab, N, n_lanes, per, t_max);
}
