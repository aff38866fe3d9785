// k_wdp.hip — depth in fixed genome windows (--window-depth; the statistic: include/bamqc.h): per read group and
// window of W bases the reads that begin in it and the covered bases of the reads of mapping quality MQ and more, and the covered bases
// of the reads below MQ.  An optional module beside k_rcv: its launch exists only when bqc_enable_window_depth has been called.  The
// genome is not read, nor any base or quality.  The products (sums by contig, the histogram) are made on the host at finalize: there is
// no second kernel.
//
// Mapping.  The walk frame of cigar_walk.h: about one workgroup per CU, WD_WAVES waves; a workgroup takes a contiguous share of the
// batch's processing order, WD_STEP reads at a time, thread t of a step fetching the fixed columns of the step's read t (those of the
// next step before this one is walked) and with them its contig's length and first window.
// The walk is k_rcv's, operation by operation, 64-bit arithmetic throughout.  A match-like operation's run [g, g + m) is clipped to
// [0, len) BEFORE its windows are looped over: what the clip takes away goes to X, a deletion or a skip costs nothing whatever its
// length, and the loop takes at most nw[rid] rounds.
// Thread path.  A read of at most WD_T operations: the operations are loaded together and walked in registers.  The loops are the
// WAVE's, not the thread's: operation q of all 64 reads is taken together, then "while any lane has a window left" each lane presents one
// add (word, bases).  That keeps the lanes in step, which the combining needs.
// Wave path.  A read of more than WD_T operations is listed in LDS (StepList) and taken by a wave, 64 operations a pass (CigWalk: the
// exact stored index j and genome position g of every operation); every lane with a match-like operation then presents that
// operation's windows in the same loop.
// Combining (wd_add).  In a sorted file the 64 reads of a wave lie in one or two windows, and the operations of a long read lie side by
// side: neighbouring lanes add to the same word.  A word is (read group, plane, window) — the index into the state, so two lanes of
// different read groups or classes never share one.  The lanes' adds are summed over RUNS of equal words among the lanes that have an
// add (a segmented sum: the runs' first lanes from one ballot, six shuffle steps) and the first lane of a run adds the run's sum: one
// atomic a run.  The default rule skips the six steps in a wave where no lane's word is that of the lane with an add below it
// (shuffled input), which the one ballot already says.
// BQC_WDP_COMBINE=0 never combines, =2 takes the six steps in every wave; all three give the same words (sums modulo 2^64 commute).
// E, E_low, X.  Three words a read group: a wave sums them over its lanes by read group and hands them to eta_add (read groups below
// WD_ETA_LANES in LDS, the others in memory).
#include "cigar_walk.h"

#define WD_THREADS 1024
#define WD_WAVES (WD_THREADS / WAVE)
#define WD_STEP WD_THREADS           // reads whose columns a workgroup fetches at a time, one per thread
#define WD_T 8                       // operations up to which a read is walked by a thread
#define WD_ETA_LANES 64              // read groups whose E, E_low, X a workgroup sums in LDS
#define WD_NONE WALK_NONE
static_assert(WD_ETA_LANES == ETA_LANES, "the E, E_low, X table of cigar_walk.h");

// floor(g / W) by a multiply and a shift.  With l = ceil(log2 W), shift = 31 + l and mul = ceil(2^shift / W): mul * W = 2^shift + e with
// 0 <= e < W <= 2^l, so g * mul / 2^shift = g / W + g e / (W 2^shift), and the second term is below 1 / W for every g < 2^31: the
// floor is exact for 0 <= g <= 2^31 - 1 and every W of 1 ... 2^24, a power of two or not.  mul < 2^32 and g * mul < 2^63: no overflow.
__device__ __forceinline__ uint32_t wd_div(const WdpTab& t, uint32_t g) { return (uint32_t)(((uint64_t)g * t.mul) >> t.shift); }

// Read i of the processing order (r == WD_NONE: not examined)
struct WdRead { uint32_t r, L, nc, coff, lane, len, woff; int32_t pos; bool good; };
__device__ __forceinline__ WdRead wd_fetch(const DevBatch& b, const WdpTab& t, uint64_t i, uint32_t end, uint32_t n_lanes, uint32_t MQ)
{
    WdRead o{WD_NONE, 0u, 0u, 0u, 0u, 0u, 0u, 0, false};
    const uint32_t r = batch_read(b, i, end);
    if (r == WALK_NONE) return o;
    const uint32_t f = b.flag[r], L = b.l_seq[r], g = b.lane[r], nc = b.n_cigar[r], mq = b.mapq[r];
    const int32_t rid = b.rid[r];
    if ((f & 0xF04u) || !L || !nc || g >= n_lanes || rid < 0 || (uint32_t)rid >= t.n_refs) return o;
    o.r = r; o.L = L; o.nc = nc; o.lane = g;
    o.coff = b.cigar_off[r];
    o.len = t.len[rid];   // (0 <= rid < n_refs: inside both tables)
    o.woff = t.woff[rid];
    o.pos = b.pos[r];
    o.good = mq >= MQ;
    return o;
}

// state[key] += val for every lane with act; the WHOLE WAVE calls.  mode 0: the adds of a run of lanes with one key become one add, in a
// wave that has such a run; 1: never; 2: the sum is taken in every wave.  A run is over the lanes WITH an add: a lane without one
// between two lanes of one key does not part them (every other operation of a long read is an insertion or a deletion, and a read
// that is not examined lies between two that are).  val <= 2^24 and a run has at most 64 lanes: the sum fits 32 bits.  key: the
// caller's bounds.
__device__ __forceinline__ void wd_add(bool act, uint32_t key, uint32_t val, uint64_t* state, uint32_t mode)
{
    if (mode == 1u) {
        if (act) gadd(state + key, val);
        return;
    }
    const uint32_t ln = (uint32_t)lane_id();
    const uint64_t am = __ballot(act);
    const uint64_t below = am & ((1ull << ln) - 1ull);
    const uint32_t pl = below ? 63u - (uint32_t)__builtin_clzll((unsigned long long)below) : ln; // the nearest lane below with an add
    const uint32_t kp = (uint32_t)__shfl((int)key, (int)pl);
    const bool head = act && (!below || kp != key); // the first lane of a run
    const uint64_t hm = __ballot(head);
    if (!act) val = 0u;
    if (mode == 2u || hm != am) { // (hm == am: every add is a run of its own, nothing to sum)
        const uint64_t H = hm | 1ull; // (the lanes in front of the first add: a run of zeros that nobody adds)
        const uint64_t rest = ln == 63u ? 0ull : H >> (ln + 1u);
        const uint32_t end = rest ? ln + 1u + (uint32_t)__builtin_ctzll((unsigned long long)rest) : (uint32_t)WAVE; // behind the run's last lane
#pragma unroll
        for (uint32_t o = 1; o < WAVE; o <<= 1) { // after the step, val covers the lanes ln ... min(ln + 2 o, end) - 1
            const uint32_t v = (uint32_t)__shfl_down((int)val, o);
            if (ln + o < end) val += v;
        }
    }
    if (head) gadd(state + key, val);
}

// The covered bases [lo, hi) of one operation, 0 <= lo < hi <= len where act, window by window: key0 is the word of the contig's window
// 0 in the read's plane.  lo < len, so lo / W < nw[rid] and the word lies inside the contig's run of the plane; (kw + 1) W <= len - 1 + W
// < 2^32.  The WHOLE WAVE calls.
__device__ __forceinline__ void wd_windows(bool act, uint32_t lo, uint32_t hi, uint32_t key0, const WdpTab& t, uint64_t* state, uint32_t mode)
{
    uint32_t kw = act ? wd_div(t, lo) : 0u;
    while (__ballot(act)) {
        uint32_t wend = 0, v = 0;
        if (act) {
            const uint32_t we = (kw + 1u) * t.W;
            wend = we < hi ? we : hi;
            v = wend - lo;
        }
        wd_add(act, key0 + kw, v, state, mode);
        if (act) {
            lo = wend;
            ++kw;
            act = lo < hi;
        }
    }
}

// E, E_low and X of the wave's examined reads (ex), summed by read group: one LDS or memory add per sum and read group.  x <= l_seq.
__device__ __forceinline__ void wd_eta(bool ex, uint32_t lane, bool good, uint32_t x, EtaTab s_eta, uint64_t* state, uint32_t lane_words)
{
    uint64_t m = __ballot(ex);
    while (m) {
        const int leader = __ffsll((unsigned long long)m) - 1;
        const uint32_t gl = __builtin_amdgcn_readlane(lane, leader);
        const bool same = ex && lane == gl;
        const uint64_t sm = __ballot(same);
        const uint64_t E = (uint64_t)__popcll((unsigned long long)__ballot(same && good)), El = (uint64_t)__popcll((unsigned long long)sm) - E;
        uint64_t X = 0;
        if (__ballot(same && x != 0u)) X = wave_sum_split(same ? x : 0u);
        if (lane_id() == leader) eta_add(s_eta, state, lane_words, gl, E, El, X);
        m &= ~sm;
    }
}

__global__ __launch_bounds__(WD_THREADS) void k_wdp(DevBatch b, WdpTab t, uint64_t* __restrict__ state, uint32_t MQ, uint32_t n_lanes, uint32_t per, uint32_t mode)
{
    __shared__ StepList<WD_STEP> s_long;                      // the long reads of a step
    __shared__ unsigned long long s_eta[WD_ETA_LANES][3];     // the workgroup's E, E_low, X by read group
    if (b.desc->fatal) return;
    const uint32_t tid = threadIdx.x, wave = tid / WAVE, ln = lane_id();
    uint32_t begin, end;
    if (!wg_share(b.n_reads, per, begin, end)) return;
    const gmem_u32* cg = (const gmem_u32*)(uintptr_t)b.cigar;
    s_long.zero();
    eta_zero(s_eta);
    block_sync();
    WdRead nx = wd_fetch(b, t, (uint64_t)begin + tid, end, n_lanes, MQ);
    StepTurn turn;
    for (uint32_t base = begin; base < end; base += WD_STEP, turn.next()) {
        const WdRead me = nx;
        if (!last_step(base, end, WD_STEP)) nx = wd_fetch(b, t, (uint64_t)base + WD_STEP + tid, end, n_lanes, MQ); // (in flight while this step is walked)
        const bool ex = me.r != WD_NONE, lng = ex && me.nc > WD_T, thr = ex && !lng;
        // the words of the read's contig: window 0 of the plane `reads` and of the read's plane of bases (lane < n_lanes and
        // woff[rid] + k < NW for a window k of the contig: inside the read group's words)
        const uint32_t rd0 = ex ? me.lane * t.lane_words + 4u + me.woff : 0u;
        const uint32_t key0 = rd0 + (me.good ? t.NW : 2u * t.NW);
        // the read's own window: a good read whose pos lies on the contig, on either path
        {
            const bool a = ex && me.good && me.pos >= 0 && (uint32_t)me.pos < me.len;
            wd_add(a, rd0 + (a ? wd_div(t, (uint32_t)me.pos) : 0u), 1u, state, mode);
        }
        // the thread path: operation q of every read of the wave together
        uint32_t w[WD_T];
#pragma unroll
        for (uint32_t k = 0; k < WD_T; ++k) w[k] = 0u;
        if (thr) {
            w[0] = cg[me.coff];
            if (me.nc > 1u) {
#pragma unroll
                for (uint32_t k = 1; k < WD_T; ++k) w[k] = k < me.nc ? cg[(uint64_t)me.coff + k] : 0u; // (cigar_off + k < the batch's operations)
            }
        }
        uint64_t j = 0;
        int64_t g = me.pos;
        bool done = !thr;
        uint32_t x = 0; // covered bases off the contig
#pragma unroll
        for (uint32_t q = 0; q < WD_T; ++q) {
            const bool has = !done && q < me.nc;
            if (!__ballot(has)) break;
            bool act = false;
            uint32_t lo = 0, hi = 0;
            if (has) {
                const uint32_t op = w[q] & 15u, n = w[q] >> 4;
                if (cig_match(op)) {
                    const uint64_t left = (uint64_t)me.L - j; // (> 0: not done)
                    const uint32_t m = n < left ? n : (uint32_t)left;
                    const int64_t a0 = g > 0 ? g : 0, a1 = g + (int64_t)m < (int64_t)me.len ? g + (int64_t)m : (int64_t)me.len;
                    if (a1 > a0) {
                        act = true;
                        lo = (uint32_t)a0;
                        hi = (uint32_t)a1;
                        x += m - (uint32_t)(a1 - a0);
                    } else x += m;
                    j += n;
                    g += (int64_t)n;
                    if (j >= me.L) done = true;
                } else if (op == 1u || op == 4u) {
                    j += n;
                    if (j >= me.L) done = true;
                } else if (op == 2u || op == 3u) {
                    g += (int64_t)n;
                }
            }
            wd_windows(act, lo, hi, key0, t, state, mode);
        }
        wd_eta(ex, me.lane, me.good, x, s_eta, state, t.lane_words); // (a long read's X follows from its wave)
        s_long.push(turn, lng, me.r); // the long reads are listed
        const uint32_t n_long = s_long.close(turn);
        // the wave path: a wave per listed read (an examined one: its columns passed wd_fetch's tests)
        for (uint32_t e = wave; e < n_long; e += WD_WAVES) {
            const uint32_t r = __builtin_amdgcn_readfirstlane(s_long.read(turn, s_long.thread(turn, e)));
            const uint32_t L = b.l_seq[r], nc = b.n_cigar[r], coff = b.cigar_off[r], rid = (uint32_t)b.rid[r], lane = b.lane[r];
            const int64_t pos = b.pos[r];
            const int64_t len = t.len[rid]; // (rid < n_refs, lane < n_lanes: wd_fetch let the read through)
            const uint32_t k0 = lane * t.lane_words + 4u + t.woff[rid] + (b.mapq[r] >= MQ ? t.NW : 2u * t.NW);
            uint32_t lx = 0;          // this lane's covered bases off the contig (their sum over the lanes is at most L)
            CigWalk<true> cw;
            cw.start(cg, coff, nc, L, pos);
            for (uint32_t p0 = 0; p0 < nc; p0 += WAVE) {
                uint32_t op, n; uint64_t jj; int64_t gg;
                cw.pass(p0, op, n, jj, gg);
                bool act = false;
                uint32_t lo = 0, hi = 0;
                if (cig_match(op) && n && jj < L) {
                    const uint64_t left = (uint64_t)L - jj;
                    const uint32_t m = n < left ? n : (uint32_t)left;
                    const int64_t a0 = gg > 0 ? gg : 0, a1 = gg + (int64_t)m < len ? gg + (int64_t)m : len;
                    if (a1 > a0) {
                        act = true;
                        lo = (uint32_t)a0;
                        hi = (uint32_t)a1;
                        lx += m - (uint32_t)(a1 - a0);
                    } else lx += m;
                }
                wd_windows(act, lo, hi, k0, t, state, mode); // (the whole wave, whatever its lanes hold)
                if (!cw.advance()) break; // (every later operation covers nothing)
            }
            if (__ballot(lx != 0u)) {
                const uint64_t X = wave_sum_split(lx);
                if (ln == 0) eta_add(s_eta, state, t.lane_words, lane, 0, 0, X);
            }
        }
        if (last_step(base, end, WD_STEP)) break;
    }
    block_sync();
    eta_flush(s_eta, state, t.lane_words, n_lanes);
}

extern "C" uint64_t bqc_wdp_words(uint32_t n_lanes, uint64_t NW) { return (uint64_t)n_lanes * (4u + 3u * NW); }

// Measuring switch, read at every launch: BQC_WDP_COMBINE=0 leaves every lane's add alone, =2 takes the segmented sum in every wave.
extern "C" void bqc_launch_wdp(const DevBatch& b, const WdpTab& t, uint64_t* state, uint32_t MQ, uint32_t n_lanes, uint32_t n_cu, hipStream_t s)
{
    if (b.n_reads == 0) return;
    const uint32_t mode = env_is("BQC_WDP_COMBINE", '0') ? 1u : env_is("BQC_WDP_COMBINE", '2') ? 2u : 0u;
    uint32_t per;
    const uint32_t g = share_grid(b.n_reads, n_cu, &per);
    hipLaunchKernelGGL(k_wdp, dim3(g), dim3(WD_THREADS), 0, s, b, t, state, MQ, n_lanes, per, mode);
}
