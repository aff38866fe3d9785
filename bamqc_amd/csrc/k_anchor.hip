// k_anchor.hip — the order-dependent part of OverallNumbers::coverage (OverallNumbers.hpp:84-110) on the card.
//
// The reference keeps, per read group, two live windows of 1000 positions: `shift` (where the first one starts), the chromosome
// `id`, and — in this library's virtual coordinates — `win`, the number of windows flushed so far.  A read that enters coverage()
// at beginPos b (bamqualcheck.cpp:318-327,392,430-433 decide which do) moves the state:
//     first read:                         id = rid, shift = b
//     id != rid or b - shift > 2000:      reset   -> id = rid, shift = b, win += 2          (unsigned arithmetic: b < shift resets too)
//     1000 < b - shift < 2000:            slide   -> shift += 1000, win += 1
// and gets {win, b - shift}.  A recurrence over 600 M reads — but almost all of it is arithmetic: behind any read, b - shift lies in
// [0, 1000] (or is 2000 exactly: neither slide nor reset, "stuck"); so a read that is less than 1000 positions behind the read before
// it (same chromosome) can only stay or slide ONCE, and a whole RUN of such reads follows from the state at the run's first read in
// closed form: with x = b - shift_entry, b - shift = x if x <= 1000, else ((x - 1) mod 1000) + 1, and the slides are what was taken
// off, in thousands.  What really is sequential are the BREAKS — a read 1000 or more behind its predecessor, out of order, or on
// another chromosome: a handful per million reads of a 30x genome (chromosome ends, gaps in the assembly), every other read in sparse
// data.  So:
//   k_an_count / k_an_scan / k_an_scatter   the reads that enter coverage(), compacted in stream order (position, chromosome, index);
//                                           the batch's other per-read facts the host used to gather (generic-path reads, records
//                                           without qualities, range of chromosomes) on the way
//   k_an_bcount / k_an_scan / k_an_bscatter the breaks among them, listed; every candidate learns the number of its run
//   k_an_chain                              ONE thread walks the breaks (their operands loaded into LDS by the workgroup, 256 at a
//                                           time): state at the end of the run before, transition of the recurrence (anchor.h: an_step,
//                                           the one the host's pass uses), state the new run starts with.  More than AN_MAX_BREAKS
//                                           breaks: the batch is left to the host's recurrence (flag in the summary; the state is not
//                                           touched)
//   k_an_apply                              every candidate: closed form from its run's entry -> {window, offset}; the candidates at
//                                           which the window changes go to the boundary list the host builds the coverage tiles from
// Several read groups (the <true> instances, k_an_scatter_g and k_an_first_offs): the reference keeps one such state per read group, and
// a read's predecessor in the recurrence is the previous candidate OF ITS GROUP.  So the candidates are compacted grouped by read group (a
// counting sort: per-workgroup per-group counts, one scan, a scatter with stable ranks — eight ballots over the lane byte give the
// "same group" mask of a wave), which makes every group's candidates one contiguous segment in stream order; a break is then also the
// first candidate of a segment; k_an_chain<true> walks each group's breaks from that group's state, one workgroup per group — the same
// walk (an_walk) over other bounds; and each group gets its own first_of segment (k_an_first_offs: back to back, sized by the group's
// last window).  With one read group the <false> instances run: no grouping to pay for, the group's part of the summary is lanes[0].
// A shard that starts inside the stream (AnchorState::pending) sets each group's candidates aside up to THAT GROUP's first certain reset:
// k_an_bcount looks for it inside every pending group's segment, k_an_chain starts the group's walk there, k_an_first_offs gives every
// group its part of the batch's pending log, and k_an_apply writes the log (BQC_COV_PENDING anchors; chromosome, position and group of
// each).  The groups leave the pending state independently, in different batches or never.
// Checked against the host's recurrence (bqc_pipeline.cpp: CovPlanner) read by read on sorted, sparse, unsorted and wild inputs
// (tests/test_gpu_anchor.py, tests/test_gpu_anchor_read_groups.py, tests/test_gpu_anchor_shard_read_groups.py), and through every test that runs the program with the reader on
// the card.
#include "kernels_common.h"
#include "anchor.h"

namespace {
__device__ __forceinline__ bool an_candidate(const AnchorArgs& a, uint32_t i)
{
    return an_is_candidate(a.flag[i], a.rid[i], a.n_refs, a.main_chrom, a.lane[i], a.n_lanes);
}

// exclusive prefix of `v` over the workgroup's 256 threads, and the workgroup's total
__device__ __forceinline__ uint32_t block_excl(uint32_t v, uint32_t* wsum /* [4] */, uint32_t& total)
{
    const uint32_t inc = wave_scan_incl(v);
    block_sync();
    if (lane_id() == WAVE - 1) wsum[threadIdx.x >> 6] = inc;
    block_sync();
    uint32_t off = inc - v;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) off += wsum[w];
    total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return off;
}

// exclusive scan of blk[0, len) in place by one workgroup of 1024 threads (wsum: [16]); returns the total
__device__ __forceinline__ uint32_t scan_excl_1024(uint32_t* blk, uint32_t len, uint32_t* wsum)
{
    uint32_t carry = 0;
    for (uint32_t base = 0; base < len; base += 1024u) { // (one round for batches of up to 4 M reads and one read group)
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < len ? blk[i] : 0u;
        const uint32_t inc = wave_scan_incl(v);
        block_sync();
        if (lane_id() == WAVE - 1) wsum[threadIdx.x >> 6] = inc;
        block_sync();
        uint32_t off = inc - v, tot = 0;
        for (uint32_t w = 0; w < 16u; ++w) { if (w < (threadIdx.x >> 6)) off += wsum[w]; tot += wsum[w]; }
        if (i < len) blk[i] = carry + off;
        carry += tot;
    }
    return carry;
}

// Several read groups: the place of this thread's item among the workgroup's items with the same key (< 2^nbits, at most 256 + 1 keys),
// in thread order, behind base[key] — which is advanced past them.  The "same key" mask of the wave from nbits ballots over the key's
// bits; cnt[w][key] (zero on entry, zero again on return) carries each wave's count to the waves behind it.  Every thread of the
// 256-thread workgroup calls this (barriers).
__device__ __forceinline__ uint32_t stable_slot(bool valid, uint32_t key, uint32_t nbits, uint32_t* base, uint32_t (*cnt)[257])
{
    uint64_t m = __ballot(valid);
    for (uint32_t b = 0; b < nbits; ++b) {
        const bool bit = (key >> b) & 1u;
        const uint64_t q = __ballot(bit);
        m &= bit ? q : ~q;
    }
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t below = (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull));
    const bool leader = valid && below == 0;
    if (leader) cnt[w][key] = (uint32_t)__popcll(m);
    block_sync();
    uint32_t pos = 0;
    if (valid) { pos = base[key] + below; for (uint32_t v = 0; v < w; ++v) pos += cnt[v][key]; }
    block_sync();
    if (leader) { atomicAdd(&base[key], cnt[w][key]); cnt[w][key] = 0; }
    block_sync();
    return pos;
}

// sum of v over the 256-thread workgroup (red: [4]); every thread gets it
__device__ __forceinline__ uint32_t block_sum256(uint32_t v, uint32_t* red)
{
    v = wave_sum(v);
    block_sync();
    if (lane_id() == 0) red[threadIdx.x >> 6] = v;
    block_sync();
    return red[0] + red[1] + red[2] + red[3];
}

// a read's state inside its run: x = beginPos - shift at the run's entry (for a stuck run: - beginPos of the read that reset)
__device__ __forceinline__ void an_closed(uint32_t x, uint32_t& delta, uint32_t& slides)
{
    if (x <= BQC_VSIZE) { delta = x; slides = 0; return; }
    delta = (x - 1u) % BQC_VSIZE + 1u;
    slides = (x - delta) / BQC_VSIZE;
}
__device__ __forceinline__ void an_in_run(const AnchorRun& r, uint32_t b, uint32_t& rel, uint32_t& delta)
{
    uint32_t slides;
    if (!r.stuck) { an_closed(b - r.s_e, delta, slides); rel = r.rel_e + slides; return; }
    if (b == r.b_e) { delta = 2u * BQC_VSIZE; rel = r.rel_e; return; }
    an_closed(b - r.b_star, delta, slides); // the first read further right reset the windows
    rel = r.rel_e + 2u + slides;
}
} // namespace

// ---- candidates ------------------------------------------------------------------------------------------------------------
// <true>: several read groups — also the workgroup's candidates per read group (blk_c) and reads per bin (blk_r: bin 0 for a lane out
// of range, bin l + 1 for read group l)
template <bool G>
__global__ __launch_bounds__(256) void k_an_count(AnchorArgs a)
{
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t hc[256], hr[257];
    const uint32_t i0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (G) {
        hc[threadIdx.x] = 0; hr[threadIdx.x] = 0;
        if (threadIdx.x == 0) hr[256] = 0;
        if (a.set_aside && blockIdx.x == 0 && threadIdx.x < a.n_lanes) a.lane_fc[threadIdx.x] = 0xFFFFFFFFu; // (k_an_bcount takes the minimum)
        block_sync();
    }
    uint32_t c = 0, n_slow = 0, max_slow = 0, n_noqual = 0, s1 = 0, s2 = 0, s3 = 0;
    int32_t rmin = INT32_MAX, rmax = -1;
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t i = i0 + k;
        if (i >= a.n) break;
        const bool cand = an_candidate(a, i);
        c += cand ? 1u : 0u;
        if (G) {
            const uint32_t ln = a.lane[i];
            atomicAdd(&hr[ln < a.n_lanes ? ln + 1u : 0u], 1u);
            if (cand) atomicAdd(&hc[ln], 1u);
        }
        const uint32_t L = a.l_seq[i], f = a.flag[i];
        s1 += (L + 1u) / 2u; s2 += L; s3 += a.n_cigar[i]; // (four reads per thread: far below 2^32; summed in 64 bits from the wave on)
        if (a.no_fast || L > BQC_FAST_MAXLEN) { ++n_slow; max_slow = max(max_slow, L); }
        n_noqual += ((f & BQC_FLAG_NO_QUAL) && !(f & 0x900u) && (f & 0xC0u)) ? 1u : 0u;
        const int32_t rid = a.rid[i];
        if ((uint32_t)rid < a.n_refs) { rmin = min(rmin, rid); rmax = max(rmax, rid); }
    }
    uint32_t total;
    (void)block_excl(c, wsum, total); // (its barriers also close the histograms)
    if (threadIdx.x == 0) a.blk_a[blockIdx.x] = total;
    if (G) {
        const uint32_t nblk = gridDim.x;
        for (uint32_t l = threadIdx.x; l < a.n_lanes; l += 256u) a.blk_c[(size_t)l * nblk + blockIdx.x] = hc[l];
        for (uint32_t l = threadIdx.x; l <= a.n_lanes; l += 256u) a.blk_r[(size_t)l * nblk + blockIdx.x] = hr[l];
    }
    // the batch's other facts: the workgroup's partial results (thousands of waves adding to the same few words took longer than the
    // rest of the kernel; k_an_scan sums the workgroups')
    __shared__ unsigned long long part[4][8];
    n_slow = wave_sum(n_slow); n_noqual = wave_sum(n_noqual);
    unsigned long long t1 = s1, t2 = s2, t3 = s3;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { t1 += __shfl_xor(t1, o); t2 += __shfl_xor(t2, o); t3 += __shfl_xor(t3, o); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        max_slow = max(max_slow, (uint32_t)__shfl_xor((int)max_slow, o));
        rmin = min(rmin, __shfl_xor(rmin, o));
        rmax = max(rmax, __shfl_xor(rmax, o));
    }
    if (lane_id() == 0) {
        unsigned long long* q = part[threadIdx.x >> 6];
        q[0] = n_slow; q[1] = max_slow; q[2] = n_noqual; q[3] = (unsigned long long)(long long)rmin; q[4] = (unsigned long long)(long long)rmax; q[5] = t1; q[6] = t2; q[7] = t3;
    }
    block_sync();
    if (threadIdx.x == 0) {
        AnchorPart P;
        P.n_slow = (uint32_t)(part[0][0] + part[1][0] + part[2][0] + part[3][0]);
        P.max_slow = (uint32_t)max(max(part[0][1], part[1][1]), max(part[2][1], part[3][1]));
        P.n_noqual = (uint32_t)(part[0][2] + part[1][2] + part[2][2] + part[3][2]);
        P.rid_min = min(min((int32_t)(long long)part[0][3], (int32_t)(long long)part[1][3]), min((int32_t)(long long)part[2][3], (int32_t)(long long)part[3][3]));
        P.rid_max = max(max((int32_t)(long long)part[0][4], (int32_t)(long long)part[1][4]), max((int32_t)(long long)part[2][4], (int32_t)(long long)part[3][4]));
        P.s1 = part[0][5] + part[1][5] + part[2][5] + part[3][5];
        P.s2 = part[0][6] + part[1][6] + part[2][6] + part[3][6];
        P.s3 = part[0][7] + part[1][7] + part[2][7] + part[3][7];
        P.first_certain = 0xFFFFFFFFu;
        a.parts[blockIdx.x] = P;
    }
}

// exclusive scan of the nscan block counts blk[] by one workgroup of 1024 threads; the total goes to *total_out; nblk: workgroups of
// k_an_count (their partial facts in parts[])
// (which: 0 = the candidates' counts (several read groups: [n_lanes][nblk], group-major) — it also starts the batch's summary and sums the workgroups' partial facts into it; 1 = the
// breaks' counts — and the first certain reset, when a shard is still setting reads aside)
__global__ __launch_bounds__(1024) void k_an_scan(uint32_t* __restrict__ blk, uint32_t nscan, uint32_t nblk, AnchorSummary* __restrict__ sum, AnchorPart* __restrict__ parts, int which)
{
    __shared__ uint32_t wsum[16];
    __shared__ unsigned long long red[16][8];
    if (which == 0) {
        unsigned long long v[8] = {0, 0, 0, (unsigned long long)(long long)INT32_MAX, (unsigned long long)(long long)-1, 0, 0, 0};
        for (uint32_t i = threadIdx.x; i < nblk; i += 1024u) {
            const AnchorPart P = parts[i];
            v[0] += P.n_slow; v[1] = max(v[1], (unsigned long long)P.max_slow); v[2] += P.n_noqual;
            v[3] = (unsigned long long)(long long)min((int32_t)(long long)v[3], P.rid_min); v[4] = (unsigned long long)(long long)max((int32_t)(long long)v[4], P.rid_max);
            v[5] += P.s1; v[6] += P.s2; v[7] += P.s3;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            v[0] += __shfl_xor(v[0], o); v[2] += __shfl_xor(v[2], o); v[5] += __shfl_xor(v[5], o); v[6] += __shfl_xor(v[6], o); v[7] += __shfl_xor(v[7], o);
            v[1] = max(v[1], (unsigned long long)__shfl_xor(v[1], o));
            v[3] = (unsigned long long)(long long)min((int32_t)(long long)v[3], (int32_t)(long long)__shfl_xor(v[3], o));
            v[4] = (unsigned long long)(long long)max((int32_t)(long long)v[4], (int32_t)(long long)__shfl_xor(v[4], o));
        }
        if (lane_id() == 0) for (int k = 0; k < 8; ++k) red[threadIdx.x >> 6][k] = v[k];
        block_sync();
        if (threadIdx.x == 0) {
            AnchorSummary z{};
            z.rid_min = INT32_MAX; z.rid_max = -1; z.first_certain = 0xFFFFFFFFu;
            for (int w = 0; w < 16; ++w) {
                z.n_slow += (uint32_t)red[w][0]; z.max_len_slow = max(z.max_len_slow, (uint32_t)red[w][1]); z.n_noqual += (uint32_t)red[w][2];
                z.rid_min = min(z.rid_min, (int32_t)(long long)red[w][3]); z.rid_max = max(z.rid_max, (int32_t)(long long)red[w][4]);
                z.seq_bytes += red[w][5]; z.qual_bytes += red[w][6]; z.cigar_words += red[w][7];
            }
            *sum = z;
        }
        block_sync();
    } else {
        uint32_t fc = 0xFFFFFFFFu;
        for (uint32_t i = threadIdx.x; i < nblk; i += 1024u) fc = min(fc, parts[i].first_certain);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) fc = min(fc, (uint32_t)__shfl_xor((int)fc, o));
        if (lane_id() == 0 && fc != 0xFFFFFFFFu) atomicMin(&sum->first_certain, fc); // (sixteen waves)
    }
    uint32_t* const total_out = which == 0 ? &sum->n_cand : &sum->n_breaks;
    const uint32_t total = scan_excl_1024(blk, nscan, wsum);
    if (threadIdx.x == 0) *total_out = total;
}

// several read groups: the candidates compacted grouped by read group, stream order inside a group (workgroup = k_an_count's 1024
// reads, taken 256 at a time so that thread order is stream order)
__global__ __launch_bounds__(256) void k_an_scatter_g(AnchorArgs a)
{
    __shared__ uint32_t base[257], cnt[4][257];
    const uint32_t nblk = gridDim.x;
    for (uint32_t l = threadIdx.x; l < 257u; l += 256u) {
        base[l] = l < a.n_lanes ? a.blk_c[(size_t)l * nblk + blockIdx.x] : 0u;
        cnt[0][l] = cnt[1][l] = cnt[2][l] = cnt[3][l] = 0;
    }
    block_sync();
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t i = blockIdx.x * 1024u + k * 256u + threadIdx.x;
        const bool in = i < a.n, cand = in && an_candidate(a, i);
        const uint32_t ln = in ? a.lane[i] : 0u;
        const uint32_t j = stable_slot(cand, ln, a.lane_bits, base, cnt);
        if (cand) { a.cpos[j] = (uint32_t)a.pos[i]; a.crid[j] = a.rid[i]; a.cidx[j] = i; a.clane[j] = (uint8_t)ln; }
        else if (in) a.cov_out[i] = CovEntry{BQC_COV_NONE, 0u};
    }
}

__global__ __launch_bounds__(256) void k_an_scatter(AnchorArgs a)
{
    __shared__ uint32_t wsum[4];
    const uint32_t i0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    bool cand[4];
    uint32_t c = 0;
    for (uint32_t k = 0; k < 4u; ++k) { cand[k] = i0 + k < a.n && an_candidate(a, i0 + k); c += cand[k] ? 1u : 0u; }
    uint32_t total;
    uint32_t j = a.blk_a[blockIdx.x] + block_excl(c, wsum, total);
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t i = i0 + k;
        if (i >= a.n) break;
        if (cand[k]) { a.cpos[j] = (uint32_t)a.pos[i]; a.crid[j] = a.rid[i]; a.cidx[j] = i; ++j; }
        else a.cov_out[i] = CovEntry{BQC_COV_NONE, 0u};
    }
}

// ---- breaks ------------------------------------------------------------------------------------------------------------------
namespace {
template <bool G>
__device__ __forceinline__ bool an_break(const AnchorArgs& a, uint32_t j)
{
    if (j == 0) return true; // the batch's first candidate: its state comes from the batch before
    if (G && a.clane[j] != a.clane[j - 1]) return true; // a read group's first candidate: its state comes from the batch before too
    return a.crid[j] != a.crid[j - 1] || a.cpos[j] - a.cpos[j - 1] >= BQC_VSIZE; // (unsigned: a read in front of its predecessor is a break)
}
}
template <bool G>
__global__ __launch_bounds__(256) void k_an_bcount(AnchorArgs a)
{
    __shared__ uint32_t wsum[4];
    const uint32_t nc = a.sum->n_cand, j0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    uint32_t c = 0;
    for (uint32_t k = 0; k < 4u; ++k) c += (j0 + k < nc && an_break<G>(a, j0 + k)) ? 1u : 0u;
    uint32_t total;
    (void)block_excl(c, wsum, total);
    if (threadIdx.x == 0) a.blk_b[blockIdx.x] = total;
    if (!G && a.state->pending) { // a shard in the middle of the stream: the first read that resets the windows whatever their state
        uint32_t fc = 0xFFFFFFFFu;
        for (uint32_t k = 0; k < 4u && fc == 0xFFFFFFFFu; ++k) {
            const uint32_t j = j0 + k;
            if (j >= nc) break;
            const bool has_prev = j ? true : a.state->has_prev != 0;
            const int32_t prid = j ? a.crid[j - 1] : a.state->prev_rid;
            const uint32_t d = a.cpos[j] - (j ? a.cpos[j - 1] : a.state->prev_bp);
            if (has_prev && (a.crid[j] != prid || (d > 2u * BQC_VSIZE && d <= 0xFFFFFFFFu - 2u * BQC_VSIZE))) fc = j;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) fc = min(fc, (uint32_t)__shfl_xor((int)fc, o));
        if (lane_id() == 0 && fc != 0xFFFFFFFFu) atomicMin(&a.parts[blockIdx.x].first_certain, fc); // (the workgroup's four waves; k_an_scan takes the minimum)
    }
    if (G && a.set_aside) { // the same per read group, for the groups that are still setting aside: the predecessor is the candidate before
                            // it in the group's segment, or for the segment's first the one the group's state remembers
        uint32_t fg = 0xFFFFFFFFu, fj = 0xFFFFFFFFu; // this thread's first certain reset, and its group
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t j = j0 + k;
            if (j >= nc) break;
            const uint32_t g = a.clane[j];
            if (g == fg) continue; // (only a group's first counts)
            const AnchorState& S = a.state[g];
            if (!S.pending) continue;
            const bool inner = j != 0 && a.clane[j - 1] == g;
            const bool has_prev = inner || S.has_prev != 0;
            const int32_t prid = inner ? a.crid[j - 1] : S.prev_rid;
            const uint32_t d = a.cpos[j] - (inner ? a.cpos[j - 1] : S.prev_bp);
            if (!(has_prev && (a.crid[j] != prid || (d > 2u * BQC_VSIZE && d <= 0xFFFFFFFFu - 2u * BQC_VSIZE)))) continue;
            if (fj != 0xFFFFFFFFu) atomicMin(&a.lane_fc[fg], fj); // (a thread whose four candidates span two pending groups)
            fg = g; fj = j;
        }
        // a wave's candidates are nearly always one group's: one atomic for the wave then
        const uint64_t has = __ballot(fj != 0xFFFFFFFFu);
        if (has) {
            const uint32_t g0 = (uint32_t)__shfl((int)fg, __ffsll((long long)has) - 1);
            if (__ballot(fj != 0xFFFFFFFFu && fg != g0) == 0) {
                uint32_t m = fj;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o));
                if (lane_id() == 0) atomicMin(&a.lane_fc[g0], m);
            } else if (fj != 0xFFFFFFFFu) atomicMin(&a.lane_fc[fg], fj);
        }
    }
}
template <bool G>
__global__ __launch_bounds__(256) void k_an_bscatter(AnchorArgs a)
{
    __shared__ uint32_t wsum[4];
    const uint32_t nc = a.sum->n_cand, j0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    bool br[4];
    uint32_t c = 0;
    for (uint32_t k = 0; k < 4u; ++k) { br[k] = j0 + k < nc && an_break<G>(a, j0 + k); c += br[k] ? 1u : 0u; }
    uint32_t total;
    uint32_t r = a.blk_b[blockIdx.x] + block_excl(c, wsum, total); // breaks in front of this thread's first candidate
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t j = j0 + k;
        if (j >= nc) break;
        if (br[k]) { if (r < AN_MAX_BREAKS) a.bj[r] = j; ++r; }
        a.crun[j] = r - 1u; // (candidate 0 is a break: r >= 1)
    }
}

// ---- the chain over the breaks -----------------------------------------------------------------------------------------------
namespace {
// The breaks [b_lo, b_hi) of a segment of candidates that ends in front of c1, walked from the state `st` in front of the segment's
// first anchored candidate j_first (the break b_lo): the workgroup loads the breaks' operands into LDS, 256 at a time, and thread 0
// runs, per break, state at the end of the run before -> step of the recurrence -> the AnchorRun the new run starts with.  Every
// thread of the workgroup calls this (barriers); THREAD 0 gets the state behind the segment's last candidate and that candidate's
// window relative to st.win.
__device__ __forceinline__ AnchorState an_walk(const AnchorArgs& a, uint32_t c1, uint32_t b_lo, uint32_t b_hi, uint32_t j_first, const AnchorState& st, uint32_t& last_rel)
{
    __shared__ uint32_t s_j[256], s_b[256], s_bl[256], s_jn[256];
    __shared__ int32_t s_rid[256];
    // the state between two reads: first / id / absolute shift / windows flushed in this batch, and the run it belongs to
    bool first = st.first != 0;
    uint32_t s = st.shift, rel = 0;
    int32_t id = st.id;
    AnchorRun run{};
    for (uint32_t base = b_lo; base < b_hi; base += 256u) {
        block_sync();
        {
            const uint32_t k = base + threadIdx.x;
            if (k < b_hi) {
                const uint32_t j = a.bj[k];
                s_j[threadIdx.x] = j; s_b[threadIdx.x] = a.cpos[j]; s_rid[threadIdx.x] = a.crid[j];
                s_bl[threadIdx.x] = j > j_first ? a.cpos[j - 1] : 0u;  // the last read of the run before
                s_jn[threadIdx.x] = k + 1 < b_hi ? a.bj[k + 1] : c1;    // where this run ends
            }
        }
        block_sync();
        if (threadIdx.x == 0) {
            const uint32_t m = min(256u, b_hi - base);
            for (uint32_t t = 0; t < m; ++t) {
                const uint32_t j = s_j[t], b = s_b[t];
                if (j != j_first) { // where the run before has got to at its last read (the first read of all: the state that came in)
                    uint32_t r2, d2;
                    an_in_run(run, s_bl[t], r2, d2);
                    rel = r2; s = s_bl[t] - d2;
                }
                const uint32_t p = an_step(first, id, s, rel, s_rid[t], b);
                run.b_e = b; run.s_e = s; run.rel_e = rel; run.stuck = p == 2u * BQC_VSIZE ? 1u : 0u; run.b_star = b;
                if (run.stuck) // the first read of the run further right (reads at the same position come first: the run is sorted)
                    for (uint32_t q = j + 1; q < s_jn[t]; ++q) { const uint32_t bq = a.cpos[q]; if (bq != b) { run.b_star = bq; break; } }
                a.runs[base + t] = run;
            }
        }
    }
    uint32_t d2;
    const uint32_t bl = a.cpos[c1 - 1];
    an_in_run(run, bl, last_rel, d2);
    AnchorState out = st;
    out.first = 0; out.id = id; out.shift = bl - d2; out.pad = 0; out.win = st.win + last_rel;
    return out;
}
} // namespace

// <false>: one workgroup for the batch's one read group; also launched alone for an empty batch.  <true>: one workgroup per read group
// walks the breaks of its segment from its own state (the limit of breaks is the batch's: over it, every workgroup leaves its group's
// state alone, the set-aside fields too).  Both with the set-aside prologue and epilogue of a shard in the middle of the stream, per
// read group: the groups leave the pending state one by one, at their own first certain reset.  Both fill the group's AnchorLane on
// every path: the host reads its before / after whatever happened.
template <bool G>
__global__ __launch_bounds__(256) void k_an_chain(AnchorArgs a)
{
    const uint32_t l = G ? blockIdx.x : 0u, nb = a.sum->n_breaks, nc_all = a.sum->n_cand;
    uint32_t c0 = 0, c1 = nc_all, n_reads = a.n;
    if (G) { // the group's reads (workgroup 0: also those out of range) and where its candidates lie
        __shared__ uint32_t red[4];
        const uint32_t nl = a.n_lanes, nblk = (a.n + 1023u) / 1024u;
        uint32_t r = 0, bad = 0;
        for (uint32_t k = threadIdx.x; k < nblk; k += 256u) { r += a.blk_r[(size_t)(l + 1) * nblk + k]; if (l == 0) bad += a.blk_r[k]; }
        auto cand_at = [&](uint32_t g) { return nblk == 0 ? 0u : g < nl ? a.blk_c[(size_t)g * nblk] : nc_all; };
        c0 = cand_at(l); c1 = cand_at(l + 1);
        n_reads = block_sum256(r, red);
        bad = block_sum256(bad, red);
        if (l == 0 && threadIdx.x == 0) a.sum->n_bad = bad;
    }
    const AnchorState st = a.state[l];
    if (threadIdx.x == 0) {
        AnchorLane L{};
        L.before = st; L.after = st; L.n_cand = c1 - c0; L.n_reads = n_reads; L.cand_off = c0; // (first_off: 0, or k_an_first_offs)
        a.lanes[l] = L;
    }
    if (nb > AN_MAX_BREAKS) { if (threadIdx.x == 0) atomicOr(&a.sum->flags, AN_FLAG_TOO_MANY_BREAKS); return; }
    if (c1 == c0) return;
    // setting aside: the candidates in front of the first certain reset are pending; the chain starts AT that read — a break — from the
    // context's own state (a stream that begins there)
    uint32_t j_first = c0;
    if (st.pending) {
        const uint32_t fc = G ? a.lane_fc[l] : a.sum->first_certain;
        j_first = fc == 0xFFFFFFFFu ? c1 : fc;
        if (threadIdx.x == 0) { a.lanes[l].n_pending = j_first - c0; if (!G) a.sum->n_pending = j_first; } // (several groups: k_an_first_offs sums them)
        if (j_first == c1) { // every candidate of the batch is set aside
            if (threadIdx.x == 0) {
                AnchorState out = st;
                out.has_prev = 1; out.prev_rid = a.crid[c1 - 1]; out.prev_bp = a.cpos[c1 - 1];
                a.state[l] = out;
                a.lanes[l].after = out;
            }
            return;
        }
    }
    // (a segment's first candidate and a certain reset are breaks: the segment's anchored breaks are [crun[j_first], crun[c1 - 1]])
    uint32_t last_rel;
    AnchorState out = an_walk(a, c1, a.crun[j_first], a.crun[c1 - 1] + 1u, j_first, st, last_rel);
    if (threadIdx.x == 0) {
        if (st.pending) { out.pending = 0; out.has_prev = 1; out.prev_rid = a.crid[j_first]; out.prev_bp = a.cpos[j_first]; }
        a.state[l] = out;
        a.lanes[l].after = out;
        a.lanes[l].last_rel = last_rel;
    }
}

// several read groups: where each group's first_of segment lies — its last_rel + 1 entries (none when every candidate of the group was
// set aside), back to back in group order, so that the host's inline copy of the table's head holds every group's windows of a dense
// batch; and where each group's part of the batch's pending log lies — behind the earlier groups' (one workgroup, a thread per group)
__global__ __launch_bounds__(256) void k_an_first_offs(AnchorArgs a)
{
    __shared__ uint32_t wsum[4];
    const uint32_t l = threadIdx.x;
    const bool in = l < a.n_lanes;
    const uint32_t np = in ? a.lanes[l].n_pending : 0u;
    const uint32_t v = in && a.lanes[l].n_cand > np ? a.lanes[l].last_rel + 1u : 0u;
    uint32_t total, n_pending;
    const uint32_t off = block_excl(v, wsum, total);
    const uint32_t pbase = block_excl(np, wsum, n_pending);
    if (in) { a.lanes[l].first_off = off; a.lanes[l].pend_base = pbase; }
    if (l == 0) a.sum->n_pending = n_pending;
}

// ---- every candidate's anchor ------------------------------------------------------------------------------------------------
// closed form from its run's entry -> {window relative to ITS group's window at batch entry, offset}; the candidates at which the
// window changes go to their group's first_of segment
template <bool G>
__global__ __launch_bounds__(256) void k_an_apply(AnchorArgs a)
{
    if (a.sum->flags & AN_FLAG_TOO_MANY_BREAKS) return;
    const uint32_t nc = a.sum->n_cand, j = blockIdx.x * 256u + threadIdx.x;
    if (j >= nc) return;
    const uint32_t i = a.cidx[j];
    const AnchorLane& L = a.lanes[G ? a.clane[j] : 0u];
    const uint32_t c0 = G ? L.cand_off + L.n_pending : a.sum->n_pending; // the group's first anchored candidate
    if (j < c0) { // set aside: its place in the batch's pending log (one group: the candidates' arrays are the log)
        const uint32_t at = G ? L.pend_base + (j - L.cand_off) : j;
        a.cov_out[i] = CovEntry{BQC_COV_PENDING, at};
        if (G) { a.plog_rid[at] = a.crid[j]; a.plog_bp[at] = a.cpos[j]; a.plog_lane[at] = a.clane[j]; }
        return;
    }
    uint32_t rel, delta;
    an_in_run(a.runs[a.crun[j]], a.cpos[j], rel, delta);
    a.cov_out[i] = CovEntry{rel, delta};
    bool boundary = j == c0;
    if (j != c0) {
        uint32_t relp, dp;
        an_in_run(a.runs[a.crun[j - 1]], a.cpos[j - 1], relp, dp);
        boundary = relp != rel;
    }
    if (boundary) {
        const uint32_t at = L.first_off + rel;
        if (rel <= L.last_rel && at < a.first_cap) a.first_of[at] = i;
        else atomicOr(&a.sum->flags, AN_FLAG_BOUND_OVERFLOW);
    }
}

// ---- the processing order of a batch with several read groups ------------------------------------------------------------------
// tmp[bin][blk] = reads of workgroup blk (1024 reads) in bin (0: lane >= n_lanes, l + 1: read group l)
__global__ __launch_bounds__(256) void k_lo_count(const uint8_t* __restrict__ lane, uint32_t n, uint32_t nl, uint32_t* __restrict__ tmp)
{
    __shared__ uint32_t h[257];
    h[threadIdx.x] = 0;
    if (threadIdx.x == 0) h[256] = 0;
    block_sync();
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t i = blockIdx.x * 1024u + k * 256u + threadIdx.x;
        if (i < n) { const uint32_t ln = lane[i]; atomicAdd(&h[ln < nl ? ln + 1u : 0u], 1u); }
    }
    block_sync();
    for (uint32_t b = threadIdx.x; b <= nl; b += 256u) tmp[(size_t)b * gridDim.x + blockIdx.x] = h[b];
}
__global__ __launch_bounds__(1024) void k_lo_scan(uint32_t* __restrict__ tmp, uint32_t len)
{
    __shared__ uint32_t wsum[16];
    (void)scan_excl_1024(tmp, len, wsum);
}
__global__ __launch_bounds__(256) void k_lo_scatter(const uint8_t* __restrict__ lane, uint32_t n, uint32_t nl, uint32_t nbits, const uint32_t* __restrict__ tmp,
                                                    uint32_t* __restrict__ order)
{
    __shared__ uint32_t base[257], cnt[4][257];
    for (uint32_t b = threadIdx.x; b < 257u; b += 256u) {
        base[b] = b <= nl ? tmp[(size_t)b * gridDim.x + blockIdx.x] : 0u;
        cnt[0][b] = cnt[1][b] = cnt[2][b] = cnt[3][b] = 0;
    }
    block_sync();
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t i = blockIdx.x * 1024u + k * 256u + threadIdx.x;
        const uint32_t ln = i < n ? lane[i] : 0u;
        const uint32_t at = stable_slot(i < n, ln < nl ? ln + 1u : 0u, nbits, base, cnt);
        if (i < n) order[at] = i;
    }
}

static uint32_t bits_for(uint32_t max_key) { return max_key ? 32u - (uint32_t)__builtin_clz(max_key) : 0u; }

extern "C" void bqc_launch_lane_order(const uint8_t* lane, uint32_t n, uint32_t nl, uint32_t* order, uint32_t* tmp, hipStream_t s)
{
    if (!n) return;
    const uint32_t nblk = (n + 1023u) / 1024u;
    hipLaunchKernelGGL(k_lo_count, dim3(nblk), dim3(256), 0, s, lane, n, nl, tmp);
    hipLaunchKernelGGL(k_lo_scan, dim3(1), dim3(1024), 0, s, tmp, nblk * (nl + 1u));
    hipLaunchKernelGGL(k_lo_scatter, dim3(nblk), dim3(256), 0, s, lane, n, nl, bits_for(nl), tmp, order);
}

template <bool G>
static void launch_anchor(const AnchorArgs& a, hipStream_t s)
{
    const uint32_t nblk = (a.n + 1023u) / 1024u; // (also the grid of the candidates' passes: n_cand <= n is only known on the card)
    if (a.n) hipLaunchKernelGGL(k_an_count<G>, dim3(nblk), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_an_scan, dim3(1), dim3(1024), 0, s, G ? a.blk_c : a.blk_a, G ? nblk * a.n_lanes : nblk, nblk, a.sum, a.parts, 0); // (starts the summary)
    if (a.n) {
        hipLaunchKernelGGL(G ? k_an_scatter_g : k_an_scatter, dim3(nblk), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_an_bcount<G>, dim3(nblk), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_an_scan, dim3(1), dim3(1024), 0, s, a.blk_b, nblk, nblk, a.sum, a.parts, 1);
        hipLaunchKernelGGL(k_an_bscatter<G>, dim3(nblk), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(k_an_chain<G>, dim3(G ? a.n_lanes : 1u), dim3(256), 0, s, a); // (an empty batch: fills the groups' state fields)
    if (a.n) {
        if (G) hipLaunchKernelGGL(k_an_first_offs, dim3(1), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_an_apply<G>, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a);
    }
}

extern "C" void bqc_launch_anchor(const AnchorArgs& a_in, hipStream_t s)
{
    AnchorArgs a = a_in;
    if (a.n_lanes > 1) { a.lane_bits = bits_for(a.n_lanes - 1u); launch_anchor<true>(a, s); } // several read groups
    else launch_anchor<false>(a, s);
}
