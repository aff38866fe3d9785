// k_sac.hip — allele counts at given sites (--site-alleles; the statistic: include/bamqc.h): per read group and
// site of a sorted list T[lane][site][4 * strand + base] counts the reads that show A, C, G or T there.  An optional module beside
// k_ibc and k_sbc: its launch exists only when bqc_enable_site_alleles has been called.  The genome is not read.
//
// A join, not a walk of every read: most reads touch no site, so the common path rejects a read in a few loads and only the rest is
// walked.
// Mapping.  The walk frame of cigar_walk.h: about one workgroup per CU, SA_WAVES waves; a workgroup takes a contiguous share of the
// batch's processing order, SA_STEP reads at a time, thread t of a step fetching the fixed columns of the step's read t (those of the
// next step before this one is looked at).
// The first site of a read.  sa_find: the contig's buckets of 4096 bases hold the index of the first site at or behind the bucket's
// start (and one entry more: the contig's end of run), so the first site >= pos is one index load and a binary search inside the
// bucket, at most 12 steps.  A read on a contig without sites or behind the contig's last bucket is rejected on the offsets alone.
// (mode 1, a measuring switch: a plain binary search over the contig's whole run instead.)
// Common path.  Reject on flags / mapq / lane / rid, find s0, and where the CIGAR is one match-like operation compare site_pos[s0]
// with pos + min(n, L).  No LDS atomic and no barrier beyond the step's one on this path: a wave without a survivor touches no LDS.
// Hit path.  The survivors of a wave are listed in LDS (StepList, two lists with one payload), so that behind the
// step's barrier threads 0 .. hits - 1 walk one listed read each: the CIGAR (at most SA_T operations, loaded together) merged with the
// site run from s0 on, 64-bit arithmetic throughout.  A deletion or skip that passes the next site looks the next one up through the
// index again instead of stepping over the sites below it.
// Wave path.  A read of more than SA_T operations is listed apart and taken by a wave, 64 operations a pass (the exact stored
// index j AND genome position g of every operation, CigWalk's arithmetic written out here); every lane with a match-like operation looks up and takes that operation's
// sites.  The read is left once the carry of j has reached L, or the carry of g has passed the contig's last site.
// Counts go to device memory with gadd: they are few and scattered by construction.
#include "cigar_walk.h"

#define SA_THREADS 1024
#define SA_WAVES (SA_THREADS / WAVE)
#define SA_STEP SA_THREADS           // reads whose columns a workgroup fetches at a time, one per thread
#define SA_T 8                       // operations up to which a read is walked by a thread
#define SA_BUCKET_SHIFT 12           // a bucket of the index: 4096 bases
#define SA_NONE WALK_NONE
#define SA_POS_MAX 0x7FFFFFFEll      // the highest position of a site

// Read i of the processing order (r == SA_NONE: not examined)
struct SaRead { uint32_t r, L, nc, coff; int32_t rid, pos; };
__device__ __forceinline__ SaRead sa_fetch(const DevBatch& b, uint64_t i, uint32_t end, uint32_t n_lanes, uint32_t n_refs, uint32_t MQ)
{
    SaRead o{SA_NONE, 0u, 0u, 0u, 0, 0};
    const uint32_t r = batch_read(b, i, end);
    if (r == WALK_NONE) return o;
    const uint32_t f = b.flag[r], L = b.l_seq[r], g = b.lane[r], nc = b.n_cigar[r], mq = b.mapq[r];
    const int32_t rid = b.rid[r];
    if ((f & 0xF04u) || (f & BQC_FLAG_NO_QUAL) || mq < MQ || !L || !nc || g >= n_lanes || rid < 0 || (uint32_t)rid >= n_refs) return o;
    o.r = r; o.L = L; o.nc = nc;
    o.coff = b.cigar_off[r];
    o.rid = rid;
    o.pos = b.pos[r];
    return o;
}

// The first site of contig rid at or behind genome position g (send: none), and send = the end of the contig's run of sites.
__device__ __forceinline__ uint32_t sa_find(const SacSites& st, uint32_t rid, int64_t g, uint32_t mode, uint32_t& send)
{
    send = st.first[rid + 1];
    if (g > SA_POS_MAX) return send;
    const int32_t x = g < 0 ? 0 : (int32_t)g;
    uint32_t lo, hi;
    if (mode) {
        lo = st.first[rid];
        hi = send;
    } else {
        const uint32_t off = st.bkt_off[rid], nb = st.bkt_off[rid + 1] - off; // entries of the contig: its buckets and one more, or none
        const uint32_t bk = (uint32_t)x >> SA_BUCKET_SHIFT;
        if (bk + 1u >= nb) return send;
        lo = st.bkt[off + bk];
        hi = st.bkt[off + bk + 1u];
    }
    while (lo < hi) { // (hi - lo <= 4096 with the index: 12 steps)
        const uint32_t mid = (lo + hi) >> 1;
        if (st.pos[mid] < x) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// what a hit path knows of its read
struct SaHit { uint32_t L, nc, coff, soff, qoff, rid, strand; int64_t pos; uint64_t* row; }; // row: T[lane]
__device__ __forceinline__ SaHit sa_hit(const DevBatch& b, uint32_t r, uint64_t* tab, uint32_t S)
{
    SaHit h;
    h.L = b.l_seq[r]; h.nc = b.n_cigar[r]; h.coff = b.cigar_off[r]; h.soff = b.seq_off[r]; h.qoff = b.qual_off[r];
    h.rid = (uint32_t)b.rid[r];
    h.strand = ((uint32_t)b.flag[r] >> 4) & 1u;
    h.pos = b.pos[r];
    h.row = tab + (uint64_t)b.lane[r] * S * 8u;
    return h;
}

// the stored base i (< L) of the read at site s
__device__ __forceinline__ void sa_count(const DevBatch& b, const SaHit& h, uint32_t s, uint64_t i, uint32_t Q)
{
    const uint32_t byte = b.seq[(uint64_t)h.soff + (i >> 1)], q = b.qual[(uint64_t)h.qoff + i];
    const uint32_t base = lut5(LUT5_FWD, (i & 1u) ? byte & 15u : byte >> 4);
    if (base < 4u && q >= Q && q <= 222u) gadd(h.row + (uint64_t)s * 8u + 4u * h.strand + base, 1);
}

__global__ __launch_bounds__(SA_THREADS) void k_sac(DevBatch b, SacSites st, uint64_t* __restrict__ tab, uint32_t Q, uint32_t MQ, uint32_t n_lanes, uint32_t per, uint32_t t_max, uint32_t mode)
{
    __shared__ struct {                                        // (one object: the compiler pads every LDS object of this size to 16 bytes)
        StepList<SA_STEP, 2> hit;                              // the survivors of a step by path: list 0 the thread path's, 1 the wave path's
        uint32_t s0[2][SA_STEP];                               // their first sites, by thread
    } s_mem;
    auto& s_hit = s_mem.hit;
    auto& s_s0 = s_mem.s0;
    if (b.desc->fatal) return;
    const uint32_t tid = threadIdx.x, wave = tid / WAVE, ln = lane_id();
    uint32_t begin, end;
    if (!wg_share(b.n_reads, per, begin, end)) return;
    const gmem_u32* cg = (const gmem_u32*)(uintptr_t)b.cigar;
    s_hit.zero();
    block_sync();
    SaRead nx = sa_fetch(b, (uint64_t)begin + tid, end, n_lanes, st.n_refs, MQ);
    StepTurn turn;
    for (uint32_t base = begin; base < end; base += SA_STEP, turn.next()) {
        const SaRead me = nx;
        if (!last_step(base, end, SA_STEP)) nx = sa_fetch(b, (uint64_t)base + SA_STEP + tid, end, n_lanes, st.n_refs, MQ); // (in flight while this step is looked at)
        // the common path
        bool hit = false;
        uint32_t s0 = 0;
        if (me.r != SA_NONE) {
            uint32_t send;
            s0 = sa_find(st, (uint32_t)me.rid, me.pos, mode, send);
            hit = s0 < send;
            if (hit && me.nc == 1u) { // one operation: no walk is needed to know the alignment's end
                const uint32_t wd = cg[me.coff], n = wd >> 4;
                hit = cig_match(wd & 15u) && (int64_t)st.pos[s0] < (int64_t)me.pos + (int64_t)min(n, me.L);
            }
        }
        const bool lng = hit && me.nc > t_max;
        if (hit) s_s0[turn.par][tid] = s0;
        s_hit.push(turn, hit, me.r, lng ? 1u : 0u);
        const uint32_t n_thr = s_hit.close(turn), n_long = s_hit.count(turn, 1);
        // the hit path: a thread per listed read
        if (tid < n_thr) {
            const uint32_t t = s_hit.thread(turn, tid, 0);
            const SaHit h = sa_hit(b, s_hit.read(turn, t), tab, st.S);
            uint32_t s = s_s0[turn.par][t], send = st.first[h.rid + 1u];
            uint32_t w[SA_T];
#pragma unroll
            for (uint32_t k = 0; k < SA_T; ++k) w[k] = k < h.nc ? cg[(uint64_t)h.coff + k] : 0u; // (0: M of no bases, which does nothing)
            uint64_t j = 0;
            int64_t g = h.pos, p = st.pos[s];
            bool done = false;
            auto step = [&](uint32_t wd) {
                const uint32_t op = wd & 15u, n = wd >> 4;
                if (done) return;
                if (cig_match(op)) {
                    const int64_t gend = g + (int64_t)n;
                    while (p < gend) { // (p >= g: the sites below g have been passed)
                        const uint64_t i = j + (uint64_t)(p - g);
                        if (i >= h.L) { done = true; break; }
                        sa_count(b, h, s, i, Q);
                        if (++s >= send) { done = true; break; }
                        p = st.pos[s];
                    }
                    j += n;
                    g = gend;
                    if (j >= h.L) done = true;
                } else if (op == 1u || op == 4u) {
                    j += n;
                    if (j >= h.L) done = true;
                } else if (op == 2u || op == 3u) {
                    g += (int64_t)n;
                    if (p < g) {
                        uint32_t e;
                        s = sa_find(st, h.rid, g, mode, e);
                        if (s >= send) done = true;
                        else p = st.pos[s];
                    }
                }
            };
#pragma unroll
            for (uint32_t k = 0; k < SA_T; ++k) step(w[k]);
            if (t_max > SA_T) // (a launch that sends longer CIGARs down this path: tools/sac_time.py's comparison)
                for (uint32_t k = SA_T; k < h.nc && !done; ++k) step(cg[(uint64_t)h.coff + k]);
        }
        // the wave path: a wave per listed read
        for (uint32_t e = wave; e < n_long; e += SA_WAVES) {
            const uint32_t r = __builtin_amdgcn_readfirstlane(s_hit.read(turn, s_hit.thread(turn, e, 1)));
            const SaHit h = sa_hit(b, r, tab, st.S);
            const uint32_t L = h.L;
            const int64_t last = st.pos[st.first[h.rid + 1u] - 1u]; // (the read is listed: the contig has a site)
            // The pass is written out here, not taken from CigWalk (cigar_walk.h, which explains the scans): with the helper this kernel's
            // long reads measured 1 to 3 % slower than before, with its own loop they do not.
            uint64_t cj = 0, cgp = 0; // the carries: bases of the read and of the genome in front of this pass
            const uint32_t nc = h.nc;
            uint32_t wd_n = ln < nc ? cg[(uint64_t)h.coff + ln] : 0u;
            for (uint32_t p0 = 0; p0 < nc; p0 += WAVE) {
                const uint32_t wd = wd_n;
                const uint32_t kn = p0 + WAVE + ln; // (nc <= 65 535: no wrap)
                wd_n = kn < nc ? cg[(uint64_t)h.coff + kn] : 0u;
                const uint32_t op = wd & 15u, n = wd >> 4, q = cig_qlen(op, n), gl = cig_glen(op, n);
                const uint32_t qlo = wave_scan_incl(q & 0xFFFFu), qhi = wave_scan_incl(q >> 16);
                const uint32_t glo = wave_scan_incl(gl & 0xFFFFu), ghi = wave_scan_incl(gl >> 16);
                const uint64_t jj = cj + (((uint64_t)qhi << 16) + qlo) - q;
                const int64_t gg = h.pos + (int64_t)(cgp + (((uint64_t)ghi << 16) + glo) - gl);
                if (cig_match(op) && n && jj < L) {
                    uint32_t send;
                    uint32_t s = sa_find(st, h.rid, gg, mode, send);
                    const int64_t gend = gg + (int64_t)n;
                    while (s < send) {
                        const int64_t p = st.pos[s];
                        if (p >= gend) break;
                        const uint64_t i = jj + (uint64_t)(p - gg);
                        if (i >= L) break;
                        sa_count(b, h, s, i, Q);
                        ++s;
                    }
                }
                cj += ((uint64_t)__builtin_amdgcn_readlane(qhi, 63) << 16) + __builtin_amdgcn_readlane(qlo, 63);
                cgp += ((uint64_t)__builtin_amdgcn_readlane(ghi, 63) << 16) + __builtin_amdgcn_readlane(glo, 63);
                if (cj >= L || h.pos + (int64_t)cgp > last) break; // (a count needs j < L and a site at or behind g)
            }
        }
        if (last_step(base, end, SA_STEP)) break;
    }
}

extern "C" uint64_t bqc_sac_words(uint32_t n_lanes, uint32_t S) { return (uint64_t)n_lanes * S * 8u; }

// Measuring switches: BQC_SAC_T=n sends reads of up to n operations down the thread path instead of SA_T; BQC_SAC_INDEX=0 replaces
// the bucket index by a binary search over the contig's whole run of sites.
extern "C" void bqc_launch_sac(const DevBatch& b, const SacSites& st, uint64_t* tab, uint32_t Q, uint32_t MQ, uint32_t n_lanes, uint32_t n_cu, hipStream_t s)
{
    if (b.n_reads == 0) return;
    static const uint32_t t_max = env_uint("BQC_SAC_T", SA_T, 65535, SA_T);
    static const uint32_t mode = env_is("BQC_SAC_INDEX", '0') ? 1u : 0u;
    uint32_t per;
    const uint32_t g = share_grid(b.n_reads, n_cu, &per);
    hipLaunchKernelGGL(k_sac, dim3(g), dim3(SA_THREADS), 0, s, b, st, tab, Q, MQ, n_lanes, per, t_max, mode);
}
