// k_rcv.hip — depth over given regions (--regions; the statistic: include/bamqc.h): per read group the reads and
// bases that land on a sorted list of disjoint regions, and the depth at every base of them, kept as a DIFFERENCE array (a run of
// covered bases adds +1 where it begins and -1 behind its end) so that the module's words stay pure sums.  An optional module beside
// k_sac: its launches exist only when bqc_enable_region_coverage has been called.  The genome is not read, nor any base or quality.
//
// k_rcv, per batch.  A join against intervals, but unlike k_sac's not one that rejects nearly every read: for a panel most reads hit,
// so there is no survivor list for the short reads: the thread that fetched a read walks it.
// Mapping.  The walk frame of cigar_walk.h: about one workgroup per CU, RC_WAVES waves; a workgroup takes a contiguous share of the
// batch's processing order, RC_STEP reads at a time, thread t of a step fetching the fixed columns of the step's read t (those of the
// next step before this one is walked).
// The first region of a base.  rc_find: "the first region of the contig with end > g", through the bucket index over the regions' ends
// (device_types.h: RcvRegions): one index load and a binary search among the regions that end inside the bucket, at most 12 steps.
// (mode 1, a measuring switch: a plain binary search over the contig's whole run instead.)
// Thread path.  A read of at most RC_T operations: the operations are loaded together and walked in registers, 64-bit arithmetic
// throughout; a CIGAR of one operation is the same code with one load.  The region index k only grows; a match-like operation whose
// region has been left behind (a deletion, a skip, or plainly the read's progress) looks k up again through the index, and then loops
// over the regions under it.  Abutting runs are not fused: a +1 and a -1 on one slot cancel in the sum.
// Wave path.  A read of more than RC_T operations is listed in LDS (StepList) and taken by a wave, 64 operations a pass (the
// exact stored index j and genome position g of every operation, CigWalk's arithmetic written out here); every lane with a match-like operation looks up and takes that
// operation's regions.
// E, T, A.  Three words a read group: a wave sums them over its lanes by read group and hands them to eta_add (read groups below
// RC_ETA_LANES in LDS, the others in memory).
// The difference words go to device memory with gadd.
//
// k_rcv_final, at bqc_finalize only, over tiles of RC_TILE slots of a read group's B + R difference words, which it only reads:
//   k_rcv_tsum   the sum of every tile;
//   k_rcv_tscan  the exclusive scan of a read group's tile sums: ONE workgroup per read group, 1024 sums a pass, the carry in a
//                register (at most 2^28 / RC_TILE = 65 536 sums, once per file: the simplest correct form);
//   k_rcv_final  per tile: thread t takes RC_PER consecutive slots, the threads' sums are scanned (waves by shuffles, the four waves'
//                totals through LDS), so every slot's prefix — the depth — is known in registers.  The region of a thread's first
//                slot comes from a binary search over off[], the following regions are stepped.  A thread folds its slots of one
//                region in registers (sum, min, max, the thresholds' counts) and hands them over with atomics when the region or its
//                slots end, so a region inside one thread's slots costs one hand-over and a region that spans threads or tiles one per
//                thread.  The histogram is privatised in LDS (u32, D + 1 <= 16384 bins; a tile adds at most RC_TILE to a bin) and added
//                to memory bin by bin where not zero.  A closing slot whose prefix is not 0 gives its region's index to an atomic min.
#include "cigar_walk.h"

#define RC_THREADS 1024
#define RC_WAVES (RC_THREADS / WAVE)
#define RC_STEP RC_THREADS           // reads whose columns a workgroup fetches at a time, one per thread
#define RC_T 8                       // operations up to which a read is walked by a thread
#define RC_BUCKET_SHIFT 12           // a bucket of the index: 4096 bases
#define RC_ETA_LANES 64              // read groups whose E, T, A a workgroup sums in LDS
#define RC_NONE WALK_NONE
#define RC_POS_MAX 0x7FFFFFFEll      // the highest base of a region
#define RC_TILE 4096                 // slots of a finalize tile
#define RC_FTHREADS 256
#define RC_PER (RC_TILE / RC_FTHREADS)
#define RC_HBINS 16384
static_assert(RC_ETA_LANES == ETA_LANES, "the E, T, A table of cigar_walk.h");

// Read i of the processing order (r == RC_NONE: not examined)
struct RcRead { uint32_t r, L, nc, coff, lane; int32_t rid, pos; };
__device__ __forceinline__ RcRead rc_fetch(const DevBatch& b, uint64_t i, uint32_t end, uint32_t n_lanes, uint32_t n_refs, uint32_t MQ)
{
    RcRead o{RC_NONE, 0u, 0u, 0u, 0u, 0, 0};
    const uint32_t r = batch_read(b, i, end);
    if (r == WALK_NONE) return o;
    const uint32_t f = b.flag[r], L = b.l_seq[r], g = b.lane[r], nc = b.n_cigar[r], mq = b.mapq[r];
    const int32_t rid = b.rid[r];
    if ((f & 0xF04u) || mq < MQ || !L || !nc || g >= n_lanes || rid < 0 || (uint32_t)rid >= n_refs) return o;
    o.r = r; o.L = L; o.nc = nc; o.lane = g;
    o.coff = b.cigar_off[r];
    o.rid = rid;
    o.pos = b.pos[r];
    return o;
}

// The first region of contig rid with end > g (send: none), and send = the end of the contig's run of regions.
__device__ __forceinline__ uint32_t rc_find(const RcvRegions& rg, uint32_t rid, int64_t g, uint32_t mode, uint32_t& send)
{
    send = rg.first[rid + 1];
    if (g > RC_POS_MAX) return send;
    const int32_t x = g < 0 ? 0 : (int32_t)g;
    uint32_t lo, hi;
    if (mode) {
        lo = rg.first[rid];
        hi = send;
    } else {
        const uint32_t off = rg.bkt_off[rid], nb = rg.bkt_off[rid + 1] - off; // entries of the contig: its buckets and one more, or none
        const uint32_t bk = (uint32_t)x >> RC_BUCKET_SHIFT;
        if (bk + 1u >= nb) return send;
        lo = rg.bkt[off + bk];       // the regions lo .. hi - 1 end inside the bucket; region hi (if any) ends behind it, so behind x
        hi = rg.bkt[off + bk + 1u];
    }
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rg.end[mid] <= x) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// The covered bases [g, gend) of one operation against the regions from k on (k < send: the first region with end > g).  Leaves k at
// the first region that may still hold a base at or behind gend.
__device__ __forceinline__ bool rc_cover(const RcvRegions& rg, uint64_t* diff, uint32_t& k, uint32_t send, int64_t g, int64_t gend)
{
    bool hit = false;
    while (k < send) {
        const int64_t s = rg.start[k], e = rg.end[k];
        if (s >= gend) break;
        const int64_t lo = g > s ? g : s, hi = gend < e ? gend : e;
        uint64_t* p = diff + rg.off[k];
        gadd(p + (uint64_t)(lo - s), 1ull);
        gadd(p + (uint64_t)(hi - s), ~0ull); // (-1 modulo 2^64)
        hit = true;
        if (e > gend) break;
        ++k;
    }
    return hit;
}

// E, T and A of the wave's examined reads (ex), summed by read group: one LDS or memory add per sum and read group.  a <= l_seq.
__device__ __forceinline__ void rc_eta(bool ex, uint32_t lane, bool hit, uint32_t a, EtaTab s_eta, uint64_t* state, uint64_t lane_words)
{
    uint64_t m = __ballot(ex);
    while (m) {
        const int leader = __ffsll((unsigned long long)m) - 1;
        const uint32_t gl = __builtin_amdgcn_readlane(lane, leader);
        const bool same = ex && lane == gl;
        const uint64_t sm = __ballot(same);
        const uint64_t E = (uint64_t)__popcll((unsigned long long)sm), T = (uint64_t)__popcll((unsigned long long)__ballot(same && hit));
        const uint64_t A = wave_sum_split(same ? a : 0u);
        if (lane_id() == leader) eta_add(s_eta, state, lane_words, gl, E, T, A);
        m &= ~sm;
    }
}

__global__ __launch_bounds__(RC_THREADS) void k_rcv(DevBatch b, RcvRegions rg, uint64_t* __restrict__ state, uint32_t MQ, uint32_t n_lanes, uint32_t per, uint32_t t_max, uint32_t mode)
{
    __shared__ StepList<RC_STEP> s_long;                      // the long reads of a step
    __shared__ unsigned long long s_eta[RC_ETA_LANES][3];     // the workgroup's E, T, A by read group
    if (b.desc->fatal) return;
    const uint32_t tid = threadIdx.x, wave = tid / WAVE, ln = lane_id();
    uint32_t begin, end;
    if (!wg_share(b.n_reads, per, begin, end)) return;
    const gmem_u32* cg = (const gmem_u32*)(uintptr_t)b.cigar;
    s_long.zero();
    eta_zero(s_eta);
    block_sync();
    RcRead nx = rc_fetch(b, (uint64_t)begin + tid, end, n_lanes, rg.n_refs, MQ);
    StepTurn turn;
    for (uint32_t base = begin; base < end; base += RC_STEP, turn.next()) {
        const RcRead me = nx;
        if (!last_step(base, end, RC_STEP)) nx = rc_fetch(b, (uint64_t)base + RC_STEP + tid, end, n_lanes, rg.n_refs, MQ); // (in flight while this step is walked)
        const bool ex = me.r != RC_NONE, lng = ex && me.nc > t_max;
        // the thread path
        bool hit = false;
        uint32_t a = 0;
        if (ex && !lng) {
            uint64_t* diff = state + (uint64_t)me.lane * rg.lane_words + 4u;
            uint32_t w[RC_T];
            w[0] = cg[me.coff];
            if (me.nc > 1u) {
#pragma unroll
                for (uint32_t k = 1; k < RC_T; ++k) w[k] = k < me.nc ? cg[(uint64_t)me.coff + k] : 0u; // (0: M of no bases, which does nothing)
            }
            uint32_t send, k = rc_find(rg, (uint32_t)me.rid, me.pos, mode, send);
            uint64_t j = 0;
            int64_t g = me.pos;
            bool done = false;
            auto step = [&](uint32_t wd) {
                const uint32_t op = wd & 15u, n = wd >> 4;
                if (done) return;
                if (cig_match(op)) {
                    const uint64_t left = (uint64_t)me.L - j; // (> 0: not done)
                    const uint32_t m = n < left ? n : (uint32_t)left;
                    a += m;
                    if (m && k < send) {
                        if ((int64_t)rg.end[k] <= g) k = rc_find(rg, (uint32_t)me.rid, g, mode, send);
                        hit |= rc_cover(rg, diff, k, send, g, g + (int64_t)m);
                    }
                    j += n;
                    g += (int64_t)n;
                    if (j >= me.L) done = true;
                } else if (op == 1u || op == 4u) {
                    j += n;
                    if (j >= me.L) done = true;
                } else if (op == 2u || op == 3u) {
                    g += (int64_t)n;
                }
            };
            step(w[0]);
            if (me.nc > 1u) {
#pragma unroll
                for (uint32_t q = 1; q < RC_T; ++q) step(w[q]);
                if (t_max > RC_T) // (a launch that sends longer CIGARs down this path: tools/rcv_time.py's comparison)
                    for (uint32_t q = RC_T; q < me.nc && !done; ++q) step(cg[(uint64_t)me.coff + q]);
            }
        }
        rc_eta(ex && !lng, me.lane, hit, a, s_eta, state, rg.lane_words);
        s_long.push(turn, lng, me.r); // the long reads are listed
        const uint32_t n_long = s_long.close(turn);
        // the wave path: a wave per listed read
        for (uint32_t e = wave; e < n_long; e += RC_WAVES) {
            const uint32_t r = __builtin_amdgcn_readfirstlane(s_long.read(turn, s_long.thread(turn, e)));
            const uint32_t L = b.l_seq[r], nc = b.n_cigar[r], coff = b.cigar_off[r], rid = (uint32_t)b.rid[r], lane = b.lane[r];
            const int64_t pos = b.pos[r];
            uint64_t* diff = state + (uint64_t)lane * rg.lane_words + 4u;
            uint32_t la = 0;          // this lane's covered bases (their sum over the lanes is at most L)
            bool lhit = false;
            // The pass is written out here, not taken from CigWalk (cigar_walk.h, which explains the scans): with the helper this kernel's
            // long reads measured 1 to 3 % slower than before, with its own loop they do not.
            uint64_t cj = 0, cgp = 0; // the carries: bases of the read and of the genome in front of this pass
            uint32_t wd_n = ln < nc ? cg[(uint64_t)coff + ln] : 0u;
            for (uint32_t p0 = 0; p0 < nc; p0 += WAVE) {
                const uint32_t wd = wd_n;
                const uint32_t kn = p0 + WAVE + ln; // (nc <= 65 535: no wrap)
                wd_n = kn < nc ? cg[(uint64_t)coff + kn] : 0u;
                const uint32_t op = wd & 15u, n = wd >> 4, q = cig_qlen(op, n), gl = cig_glen(op, n);
                const uint32_t qlo = wave_scan_incl(q & 0xFFFFu), qhi = wave_scan_incl(q >> 16);
                const uint32_t glo = wave_scan_incl(gl & 0xFFFFu), ghi = wave_scan_incl(gl >> 16);
                const uint64_t jj = cj + (((uint64_t)qhi << 16) + qlo) - q;
                const int64_t gg = pos + (int64_t)(cgp + (((uint64_t)ghi << 16) + glo) - gl);
                if (cig_match(op) && n && jj < L) {
                    const uint64_t left = (uint64_t)L - jj;
                    const uint32_t m = n < left ? n : (uint32_t)left;
                    la += m;
                    uint32_t send, k = rc_find(rg, rid, gg, mode, send);
                    lhit |= rc_cover(rg, diff, k, send, gg, gg + (int64_t)m);
                }
                cj += ((uint64_t)__builtin_amdgcn_readlane(qhi, 63) << 16) + __builtin_amdgcn_readlane(qlo, 63);
                cgp += ((uint64_t)__builtin_amdgcn_readlane(ghi, 63) << 16) + __builtin_amdgcn_readlane(glo, 63);
                if (cj >= L) break; // (every later operation covers nothing)
            }
            const uint64_t A = wave_sum_split(la);
            const bool any = __ballot(lhit) != 0;
            if (ln == 0) eta_add(s_eta, state, rg.lane_words, lane, 1, any ? 1 : 0, A);
        }
        if (last_step(base, end, RC_STEP)) break;
    }
    block_sync();
    eta_flush(s_eta, state, rg.lane_words, n_lanes);
}

// ---- finalize ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t rc_wave_sum64(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o);
    return v;
}
__device__ __forceinline__ uint64_t rc_wave_scan64(uint64_t v) // inclusive
{
    const int ln = lane_id();
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint64_t t = (uint64_t)__shfl_up((unsigned long long)v, o);
        if (ln >= o) v += t;
    }
    return v;
}

// out, by read group: [R][C = 3 + n_thr: sum, min, max, ge...] then hist[D + 1]; behind all read groups one word: the first region
// whose closing slot is not 0 (~0: none).  Everything starts at 0 but the minima and that word.
__global__ void k_rcv_init(uint64_t* out, uint64_t lane_out, uint64_t RC, uint32_t C, uint64_t total)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > total) return;
    if (i == total) { out[i] = ~0ull; return; }
    const uint64_t x = i % lane_out;
    out[i] = x < RC && x % C == 1u ? ~0ull : 0ull;
}

__global__ __launch_bounds__(RC_FTHREADS) void k_rcv_tsum(const uint64_t* __restrict__ state, uint64_t lane_words, uint32_t W, uint32_t n_tiles, uint64_t* __restrict__ tsum)
{
    __shared__ uint64_t s_w[RC_FTHREADS / WAVE];
    const uint32_t tile = blockIdx.x, lane = blockIdx.y, tid = threadIdx.x;
    const uint64_t* d = state + (uint64_t)lane * lane_words + 4u;
    uint64_t v = 0;
    for (uint32_t q = 0; q < RC_PER; ++q) {
        const uint64_t x = (uint64_t)tile * RC_TILE + (uint64_t)q * RC_FTHREADS + tid;
        if (x < W) v += d[x];
    }
    v = rc_wave_sum64(v);
    if (lane_id() == 0) s_w[tid / WAVE] = v;
    block_sync();
    if (tid == 0) {
        uint64_t t = 0;
        for (uint32_t q = 0; q < RC_FTHREADS / WAVE; ++q) t += s_w[q];
        tsum[(uint64_t)lane * n_tiles + tile] = t;
    }
}

__global__ __launch_bounds__(1024) void k_rcv_tscan(uint64_t* __restrict__ tsum, uint32_t n_tiles)
{
    __shared__ uint64_t s_w[1024 / WAVE];
    uint64_t* t = tsum + (uint64_t)blockIdx.x * n_tiles;
    const uint32_t tid = threadIdx.x, wave = tid / WAVE;
    uint64_t carry = 0;
    for (uint32_t p0 = 0; p0 < n_tiles; p0 += 1024u) {
        const uint32_t i = p0 + tid;
        const uint64_t v = i < n_tiles ? t[i] : 0ull;
        const uint64_t inc = rc_wave_scan64(v);
        if (lane_id() == WAVE - 1) s_w[wave] = inc;
        block_sync();
        uint64_t before = 0, all = 0;
        for (uint32_t q = 0; q < 1024 / WAVE; ++q) {
            const uint64_t x = s_w[q];
            if (q < wave) before += x;
            all += x;
        }
        if (i < n_tiles) t[i] = carry + before + inc - v;
        carry += all;
        block_sync(); // (s_w is written again)
    }
}

__global__ __launch_bounds__(RC_FTHREADS) void k_rcv_final(const uint64_t* __restrict__ state, RcvRegions rg, RcvFinal fp, uint32_t W, uint32_t n_tiles, const uint64_t* __restrict__ tsum, uint64_t* __restrict__ out, uint64_t lane_out, uint64_t err_at)
{
    __shared__ uint32_t s_h[RC_HBINS]; // the tile's histogram; in front of it, the waves' totals of the scan in its first words
    const uint32_t tile = blockIdx.x, lane = blockIdx.y, tid = threadIdx.x, wave = tid / WAVE;
    const uint64_t* d = state + (uint64_t)lane * rg.lane_words + 4u;
    const uint32_t C = 3u + fp.n_thr, D = fp.D;
    uint64_t* reg = out + (uint64_t)lane * lane_out;
    uint64_t* hist = reg + (uint64_t)rg.R * C;
    const uint64_t x0 = (uint64_t)tile * RC_TILE + (uint64_t)tid * RC_PER; // this thread's first slot
    uint64_t v[RC_PER];
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t q = 0; q < RC_PER; ++q) {
        v[q] = x0 + q < W ? d[x0 + q] : 0ull;
        mine += v[q];
    }
    const uint64_t inc = rc_wave_scan64(mine);
    uint64_t* s_w = (uint64_t*)s_h;
    if (lane_id() == WAVE - 1) s_w[wave] = inc;
    block_sync();
    uint64_t depth = tsum[(uint64_t)lane * n_tiles + tile] + inc - mine;
    for (uint32_t q = 0; q < wave; ++q) depth += s_w[q];
    block_sync();
    for (uint32_t q = tid; q <= D; q += RC_FTHREADS) s_h[q] = 0;
    block_sync();
    if (x0 < W) {
        // the region of the first slot: the last k with off[k] <= x0 (off[0] == 0, off[R] == W > x0)
        uint32_t lo = 0, hi = rg.R;
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (rg.off[mid] <= x0) lo = mid;
            else hi = mid;
        }
        uint32_t k = lo;
        uint64_t close = (uint64_t)rg.off[k + 1u] - 1u; // the region's closing slot
        uint64_t sum = 0, mn = ~0ull, mx = 0;
        uint32_t ge[BQC_RCV_MAX_THRESHOLDS], n = 0;
#pragma unroll
        for (uint32_t t = 0; t < BQC_RCV_MAX_THRESHOLDS; ++t) ge[t] = 0;
        auto hand = [&]() {
            if (!n) return;
            uint64_t* r = reg + (uint64_t)k * C;
            gadd(r, sum);
            __hip_atomic_fetch_min((gmem_u64*)(uintptr_t)(r + 1), (unsigned long long)mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max((gmem_u64*)(uintptr_t)(r + 2), (unsigned long long)mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (uint32_t t = 0; t < BQC_RCV_MAX_THRESHOLDS; ++t)
                if (t < fp.n_thr && ge[t]) gadd(r + 3u + t, ge[t]);
            sum = 0; mn = ~0ull; mx = 0; n = 0;
#pragma unroll
            for (uint32_t t = 0; t < BQC_RCV_MAX_THRESHOLDS; ++t) ge[t] = 0;
        };
#pragma unroll
        for (uint32_t q = 0; q < RC_PER; ++q) {
            const uint64_t x = x0 + q;
            if (x < W) {
                depth += v[q];
                if (x == close) {
                    if (depth) __hip_atomic_fetch_min((gmem_u64*)(uintptr_t)(out + err_at), (unsigned long long)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    hand();
                    ++k;
                    if (k < rg.R) close = (uint64_t)rg.off[k + 1u] - 1u;
                } else {
                    sum += depth;
                    mn = depth < mn ? depth : mn;
                    mx = depth > mx ? depth : mx;
                    ++n;
#pragma unroll
                    for (uint32_t t = 0; t < BQC_RCV_MAX_THRESHOLDS; ++t) ge[t] += (t < fp.n_thr && depth >= fp.thr[t]) ? 1u : 0u;
                    atomicAdd(&s_h[depth < D ? (uint32_t)depth : D], 1u);
                }
            }
        }
        hand();
    }
    block_sync();
    for (uint32_t q = tid; q <= D; q += RC_FTHREADS) {
        const uint32_t c = s_h[q];
        if (c) gadd(hist + q, c);
    }
}

extern "C" uint64_t bqc_rcv_words(uint32_t n_lanes, uint64_t B, uint32_t R) { return (uint64_t)n_lanes * (4u + B + R); }
extern "C" uint32_t bqc_rcv_tiles(uint64_t B, uint32_t R) { return (uint32_t)((B + R + RC_TILE - 1) / RC_TILE); }
// the words of bqc_launch_rcv_final's `out`
extern "C" uint64_t bqc_rcv_out_words(uint32_t n_lanes, uint32_t R, uint32_t n_thr, uint32_t D) { return (uint64_t)n_lanes * ((uint64_t)R * (3u + n_thr) + D + 1u) + 1u; }

// Measuring switches: BQC_RCV_T=n sends reads of up to n operations down the thread path instead of RC_T; BQC_RCV_INDEX=0 replaces
// the bucket index by a binary search over the contig's whole run of regions.
extern "C" void bqc_launch_rcv(const DevBatch& b, const RcvRegions& rg, uint64_t* state, uint32_t MQ, uint32_t n_lanes, uint32_t n_cu, hipStream_t s)
{
    if (b.n_reads == 0) return;
    static const uint32_t t_max = env_uint("BQC_RCV_T", RC_T, 65535, RC_T);
    static const uint32_t mode = env_is("BQC_RCV_INDEX", '0') ? 1u : 0u;
    uint32_t per;
    const uint32_t g = share_grid(b.n_reads, n_cu, &per);
    hipLaunchKernelGGL(k_rcv, dim3(g), dim3(RC_THREADS), 0, s, b, rg, state, MQ, n_lanes, per, t_max, mode);
}

// The finalize pass: `state` is read only; tsum holds n_lanes * bqc_rcv_tiles words, out bqc_rcv_out_words.
extern "C" void bqc_launch_rcv_final(const uint64_t* state, const RcvRegions& rg, const RcvFinal& fp, uint32_t n_lanes, uint64_t* tsum, uint64_t* out, hipStream_t s)
{
    const uint32_t W = (uint32_t)(rg.lane_words - 4u), n_tiles = (W + RC_TILE - 1) / RC_TILE, C = 3u + fp.n_thr;
    const uint64_t RC = (uint64_t)rg.R * C, lane_out = RC + fp.D + 1u, total = lane_out * n_lanes;
    hipLaunchKernelGGL(k_rcv_init, dim3((uint32_t)((total + 1 + 255) / 256)), dim3(256), 0, s, out, lane_out, RC, C, total);
    hipLaunchKernelGGL(k_rcv_tsum, dim3(n_tiles, n_lanes), dim3(RC_FTHREADS), 0, s, state, rg.lane_words, W, n_tiles, tsum);
    hipLaunchKernelGGL(k_rcv_tscan, dim3(n_lanes), dim3(1024), 0, s, tsum, n_tiles);
    hipLaunchKernelGGL(k_rcv_final, dim3(n_tiles, n_lanes), dim3(RC_FTHREADS), 0, s, state, rg, fp, W, n_tiles, tsum, out, lane_out, total);
}
