// k_dup.hip — duplicate sets by alignment signature (--duplicate-sets; the rule: include/bamqc.h): every examined
// read has a signature (class, strand, mate strand, rid, unclipped 5' position, tlen), two reads with equal signatures are in one set,
// and the sets are counted EXACTLY in a hash table in device memory.  An optional module beside k_rcv: its launches and its memory
// exist only when bqc_enable_duplicate_sets has been called.  The genome is not read, nor any base or quality.  The module's state is
// NOT part of the flat state vector: the table cannot be summed word by word.
//
// The table (dup_table.h: its code is shared with k_ovr.hip).  C slots (a power of two, at least twice the capacity in signatures) of DupSlot {k0, k1, count}, open addressing with
// linear probing; an empty key word is all ones (k0 has 49 bits; k1's low half is a rid >= 0).  Every access to a key word or a count
// while reads are inserted is an 8-byte agent-scope atomic: nothing is fenced, and no L1 can serve a stale key.
// The insert never waits for another thread.  At a slot: (1) k0 is loaded, and if empty claimed by a compare-and-swap; (2) if the
// slot's k0 is now this signature's, the same for k1; (3) if k1 is this signature's too the slot is the signature's, and its count is
// added to — the thread whose compare-and-swap of k1 succeeded has made a new set; (4) otherwise both words are set, stay as they
// are for good, and belong to another signature: the next slot.  k0 may be claimed by one thread and k1 by another with the same k0:
// the slot then holds the second thread's signature and the first moves on.  Every thread of one signature sees the same immutable
// words at every slot of its probe sequence, so all of them end in the same slot: no two signatures share a set, no signature has two.
// The bound.  New sets are counted per workgroup and step in LDS and added to one word behind the table once a step.  A probe sequence
// looks at that word every DP_CHECK slots and gives up when it has passed the capacity; it also gives up after C slots.  Giving up, or
// a workgroup that finds the word above the capacity at its end (the last one sees every set), sets BQC_DEVERR_DUP in the batch's
// error record: the stream fails with BQC_ERR_RANGE.  A launch that finds the word above the capacity at its start does nothing.
//
// k_dup, per batch.  The walk frame of cigar_walk.h: about one workgroup per CU, DP_WAVES waves; a workgroup takes a contiguous share
// of the batch's processing order, DP_STEP reads at a time, thread t of a step fetching the fixed columns of the step's read t (those
// of the next step before this one is inserted).
// Thread path.  A read of at most DP_T operations: its words are loaded together, lead, trail and reflen come from registers.  A
// FORWARD read of more operations needs only its leading clips: where one of its first DP_T operations is no clip, it stays here.
// Wave path.  Every other read of more than DP_T operations is listed in LDS (StepList) and taken by a wave, 64 operations a pass
// (CigWalk's loads; the sums are wave_sum_split's, exact).  Lane 0 then inserts the read.
// Equal signatures of a wave are combined by ballots before the table is touched, one insert with their number — in the waves where
// some lane's signature is that of the lane beside it (mode bit 0: never; bit 2: in every wave).
// The slot of a signature is a mix of the whole signature (mode bit 1: a mix of (rid, u5 >> 6, the rest) in the high bits and u5 & 63
// in the low 6, so that sorted reads land in few rows of the table: measured, no gain).  The products do not depend on either.
// The five sums of a read group (E and F by class, the second ends) are ballots by read group, added to the workgroup's LDS copy and
// once, at the workgroup's end, to memory.
//
// k_dup_final, at bqc_finalize only: one pass over the C slots, which it only reads: the sets by class and size into LDS histograms
// (one add a bin and workgroup to memory), the largest set by a maximum per wave.
#include "cigar_walk.h"
#include "dup_table.h" // the table: slot, claim, insert, clear (also k_ovr.hip's)

#define DP_THREADS 1024
#define DP_WAVES (DP_THREADS / WAVE)
#define DP_STEP DP_THREADS
#define DP_T 8                       // operations up to which a read's CIGAR is summed by its own thread
#define DP_LANES 256                 // read groups (the lane column is a byte)
#define DP_NONE WALK_NONE
#define DP_FTHREADS 256

// Read i of the processing order.  cls: 0 single, 1 pair, 2 second end, DP_NONE not examined
struct DpRead { uint32_t cls, r, nc, coff, lane, info; int32_t rid, pos, tlen; }; // info: strand | mate strand << 1 | flagged << 2
__device__ __forceinline__ DpRead dp_read(const DevBatch& b, uint32_t r, uint32_t n_lanes, uint32_t n_refs)
{
    DpRead o{DP_NONE, r, 0u, 0u, 0u, 0u, 0, 0, 0};
    const uint32_t f = b.flag[r], L = b.l_seq[r], g = b.lane[r], nc = b.n_cigar[r];
    const int32_t rid = b.rid[r];
    if ((f & 0xB04u) || !L || !nc || g >= n_lanes || rid < 0 || (uint32_t)rid >= n_refs) return o;
    const int32_t tlen = b.tlen[r];
    const bool both = (f & 1u) && !(f & 8u);
    o.cls = both && tlen > 0 ? 1u : both && tlen < 0 ? 2u : 0u;
    o.nc = nc; o.lane = g;
    o.coff = b.cigar_off[r];
    o.info = ((f >> 4) & 1u) | (o.cls == 1u ? (f >> 5) & 1u : 0u) << 1 | ((f >> 10) & 1u) << 2;
    o.rid = rid;
    o.pos = b.pos[r];
    o.tlen = o.cls == 1u ? tlen : 0;
    return o;
}
__device__ __forceinline__ DpRead dp_fetch(const DevBatch& b, uint64_t i, uint32_t end, uint32_t n_lanes, uint32_t n_refs)
{
    const DpRead none{DP_NONE, 0u, 0u, 0u, 0u, 0u, 0, 0, 0};
    const uint32_t r = batch_read(b, i, end);
    return r == WALK_NONE ? none : dp_read(b, r, n_lanes, n_refs);
}

__device__ __forceinline__ bool dp_clip(uint32_t op) { return op == 4u || op == 5u; }

// the two key words of a read (cls 0 or 1) from its clips and its length on the genome
__device__ __forceinline__ void dp_keys(const DpRead& me, uint64_t lead, uint64_t trail, uint64_t reflen, uint64_t& k0, uint64_t& k1)
{
    const bool rev = me.info & 1u;
    const int64_t u5 = rev ? (int64_t)me.pos + (int64_t)reflen - 1 + (int64_t)trail : (int64_t)me.pos - (int64_t)lead; // |u5| < 2^31 + 2^44
    k0 = (uint64_t)(u5 + (1ll << 45)) | (uint64_t)me.cls << 46 | (uint64_t)(me.info & 3u) << 47;
    k1 = (uint64_t)(uint32_t)me.rid | (uint64_t)(uint32_t)me.tlen << 32;
}

__global__ __launch_bounds__(DP_THREADS) void k_dup(DevBatch b, DupTable T, uint64_t* __restrict__ sums, uint32_t* __restrict__ err, uint32_t n_lanes, uint32_t n_refs, uint32_t per, uint32_t mode)
{
    __shared__ StepList<DP_STEP> s_long;                    // the long reads of a step
    __shared__ uint32_t s_new[3];                           // [step mod 3] new sets: rotated with the list's counters
    __shared__ uint32_t s_full;                             // the table went over its capacity in an earlier batch
    __shared__ unsigned long long s_sum[DP_LANES][5];       // the workgroup's sums by read group
    if (b.desc->fatal) return;
    if (threadIdx.x == 0) s_full = dp_load(T.n_sets) > T.capacity ? 1u : 0u;
    block_sync();
    if (s_full) return;                                     // (the stream has failed; one thread looks, so the whole workgroup leaves or stays)
    const uint32_t tid = threadIdx.x, wave = tid / WAVE, ln = lane_id();
    uint32_t begin, end;
    if (!wg_share(b.n_reads, per, begin, end)) return;
    const gmem_u32* cg = (const gmem_u32*)(uintptr_t)b.cigar;
    s_long.zero();
    if (tid < 3) s_new[tid] = 0;
    for (uint32_t t = tid; t < DP_LANES * 5; t += DP_THREADS) s_sum[t / 5][t % 5] = 0;
    block_sync();
    bool over = false;
    DpRead nx = dp_fetch(b, (uint64_t)begin + tid, end, n_lanes, n_refs);
    StepTurn turn;
    for (uint32_t base = begin; base < end; base += DP_STEP, turn.next()) {
        const DpRead me = nx;
        if (!last_step(base, end, DP_STEP)) nx = dp_fetch(b, (uint64_t)base + DP_STEP + tid, end, n_lanes, n_refs); // (in flight while this step is inserted)
        const bool ex = me.cls != DP_NONE, need = ex && me.cls < 2u, rev = me.info & 1u;
        // the sums, by read group
        {
            uint64_t m = __ballot(ex);
            while (m) {
                const int leader = __ffsll((unsigned long long)m) - 1;
                const uint32_t gl = __builtin_amdgcn_readlane(me.lane, leader);
                const bool same = ex && me.lane == gl;
                const uint64_t sm = __ballot(same);
                const bool fl = (me.info >> 2) & 1u;
                const uint32_t e0 = (uint32_t)__popcll((unsigned long long)__ballot(same && me.cls == 0u)), e1 = (uint32_t)__popcll((unsigned long long)__ballot(same && me.cls == 1u));
                const uint32_t f0 = (uint32_t)__popcll((unsigned long long)__ballot(same && me.cls == 0u && fl)), f1 = (uint32_t)__popcll((unsigned long long)__ballot(same && me.cls == 1u && fl));
                const uint32_t se = (uint32_t)__popcll((unsigned long long)__ballot(same && me.cls == 2u));
                if ((int)ln == leader) {
                    if (e0) atomicAdd(&s_sum[gl][0], (unsigned long long)e0);
                    if (e1) atomicAdd(&s_sum[gl][1], (unsigned long long)e1);
                    if (f0) atomicAdd(&s_sum[gl][2], (unsigned long long)f0);
                    if (f1) atomicAdd(&s_sum[gl][3], (unsigned long long)f1);
                    if (se) atomicAdd(&s_sum[gl][4], (unsigned long long)se);
                }
                m &= ~sm;
            }
        }
        // the thread path: the first DP_T operations
        uint64_t lead = 0, trail = 0, reflen = 0;
        bool pre = true;
        if (need) {
            uint32_t w[DP_T];
            w[0] = cg[me.coff];
            if (me.nc > 1u) {
#pragma unroll
                for (uint32_t k = 1; k < DP_T; ++k) w[k] = k < me.nc ? cg[(uint64_t)me.coff + k] : 0u;
            }
#pragma unroll
            for (uint32_t k = 0; k < DP_T; ++k) {
                if (k < me.nc) {
                    const uint32_t op = w[k] & 15u, n = w[k] >> 4;
                    if (dp_clip(op)) { if (pre) lead += n; else trail += n; }
                    else { pre = false; trail = 0; reflen += cig_glen(op, n); }
                }
            }
        }
        const bool lng = need && me.nc > DP_T && (rev || pre);
        bool ins = need && !lng;
        uint64_t k0 = 0, k1 = 0, n = 1;
        if (ins) dp_keys(me, lead, trail, reflen, k0, k1);
        // equal signatures of the wave: the first lane of each takes them all — where a lane's signature is its neighbour's (sorted
        // input: duplicates arrive side by side; a wave of different signatures skips the loop, which costs it more than it saves)
        const uint32_t digest = ins ? (uint32_t)k0 ^ (uint32_t)(k0 >> 32) ^ (uint32_t)k1 * 0x9E3779B1u ^ (uint32_t)(k1 >> 32) : ln;
        const bool beside = ins && ln > 0 && (uint32_t)__shfl_up((int)digest, 1) == digest;
        if ((mode & 4u) || (!(mode & 1u) && __ballot(beside))) {
            uint64_t m = __ballot(ins);
            while (m) {
                const int leader = __ffsll((unsigned long long)m) - 1;
                const uint32_t a0 = __builtin_amdgcn_readlane((uint32_t)k0, leader), a1 = __builtin_amdgcn_readlane((uint32_t)(k0 >> 32), leader);
                const uint32_t b0 = __builtin_amdgcn_readlane((uint32_t)k1, leader), b1 = __builtin_amdgcn_readlane((uint32_t)(k1 >> 32), leader);
                const bool same = ins && (uint32_t)k0 == a0 && (uint32_t)(k0 >> 32) == a1 && (uint32_t)k1 == b0 && (uint32_t)(k1 >> 32) == b1;
                const uint64_t sm = __ballot(same);
                if ((int)ln == leader) n = (uint64_t)__popcll((unsigned long long)sm);
                else if (same) ins = false;
                m &= ~sm;
            }
        }
        uint32_t fresh = 0;
        if (ins) fresh = dp_insert(T, k0, k1, n, mode, over);
        {
            const uint64_t fm = __ballot(fresh != 0u);
            if (fm && ln == 0) atomicAdd(&s_new[turn.cnt], (uint32_t)__popcll((unsigned long long)fm));
        }
        s_long.push(turn, lng, me.r); // the long reads are listed
        const uint32_t n_long = s_long.close(turn);
        if (tid == 0) { // the step before's new sets: added to last in front of this barrier, added to again behind the next
            const uint32_t pv = turn.prev(), v = s_new[pv];
            if (v) gadd(T.n_sets, v);
            s_new[pv] = 0;
        }
        // the wave path: a wave per listed read
        for (uint32_t e = wave; e < n_long; e += DP_WAVES) {
            const DpRead rd = dp_read(b, __builtin_amdgcn_readfirstlane(s_long.read(turn, s_long.thread(turn, e))), n_lanes, n_refs);
            const uint32_t nc = __builtin_amdgcn_readfirstlane(rd.nc), coff = __builtin_amdgcn_readfirstlane(rd.coff);
            const bool rv = __builtin_amdgcn_readfirstlane(rd.info) & 1u;
            uint64_t ld = 0, tr = 0, rl = 0;
            bool pr = true;
            CigWalk<false> cw;
            cw.start(cg, coff, nc);
            for (uint32_t p0 = 0; p0 < nc; p0 += WAVE) {
                uint32_t op, len;
                const bool valid = cw.load(p0, op, len);
                const bool clip = valid && dp_clip(op), other = valid && !clip;
                const uint64_t ob = __ballot(other);
                const uint32_t cn = clip ? len : 0u;
                rl += wave_sum_split(other ? cig_glen(op, len) : 0u);
                if (!ob) {
                    const uint64_t tot = wave_sum_split(cn);
                    if (pr) ld += tot; else tr += tot;
                } else {
                    const uint32_t first = (uint32_t)__ffsll((unsigned long long)ob) - 1u, last = 63u - (uint32_t)__clzll((long long)ob);
                    if (pr) ld += wave_sum_split(ln < first ? cn : 0u);
                    pr = false;
                    tr = wave_sum_split(ln > last ? cn : 0u);
                }
                if (!rv && !pr) break; // (a forward read needs its leading clips only)
            }
            uint32_t fr = 0;
            if (ln == 0) {
                uint64_t q0, q1;
                dp_keys(rd, ld, tr, rl, q0, q1);
                fr = dp_insert(T, q0, q1, 1, mode, over);
                if (fr) atomicAdd(&s_new[turn.cnt], 1u);
            }
        }
        if (last_step(base, end, DP_STEP)) break;
    }
    if (over) atomicOr(err, BQC_DEVERR_DUP);
    block_sync();
    for (uint32_t t = tid; t < DP_LANES * 5; t += DP_THREADS) {
        const unsigned long long v = s_sum[t / 5][t % 5];
        if (v) gadd(sums + t, v); // (a read group with a sum is below n_lanes)
    }
    if (tid == 0) { // what is left of the counters, and the look at the whole
        const uint64_t v = (uint64_t)s_new[0] + s_new[1] + s_new[2];
        const dp_u64 before = __hip_atomic_fetch_add((gmem_u64*)(uintptr_t)T.n_sets, (dp_u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before + v > T.capacity) atomicOr(err, BQC_DEVERR_DUP);
    }
}

// ---- finalize ----------------------------------------------------------------------------------------------------------------------
// out: [2 classes][BQC_DUP_BINS] sets by size, then the two largest sets; zero before the launch.
__global__ __launch_bounds__(DP_FTHREADS) void k_dup_final(const DupSlot* __restrict__ slots, uint64_t C, uint64_t* __restrict__ out)
{
    __shared__ uint32_t s_h[2][BQC_DUP_BINS]; // (a workgroup takes fewer than 2^32 slots)
    const uint32_t tid = threadIdx.x;
    for (uint32_t t = tid; t < 2 * BQC_DUP_BINS; t += DP_FTHREADS) s_h[t / BQC_DUP_BINS][t % BQC_DUP_BINS] = 0;
    block_sync();
    uint64_t big[2] = {0, 0};
    const uint64_t step = (uint64_t)gridDim.x * DP_FTHREADS;
    for (uint64_t x = (uint64_t)blockIdx.x * DP_FTHREADS + tid; x < C; x += step) {
        const uint64_t k0 = slots[x].k0;
        if (k0 == BQC_DUP_EMPTY) continue;
        const uint64_t n = slots[x].count;
        if (!n) continue; // (never: the add follows the claim of k1; a bin below the first does not exist)
        const uint32_t cls = (uint32_t)(k0 >> 46) & 1u;
        atomicAdd(&s_h[cls][(n < BQC_DUP_BINS ? (uint32_t)n : (uint32_t)BQC_DUP_BINS) - 1u], 1u);
        big[cls] = n > big[cls] ? n : big[cls];
    }
#pragma unroll
    for (uint32_t c = 0; c < 2; ++c) {
        uint64_t v = big[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t t = (uint64_t)__shfl_xor((unsigned long long)v, o);
            v = t > v ? t : v;
        }
        if (lane_id() == 0 && v) __hip_atomic_fetch_max((gmem_u64*)(uintptr_t)(out + 2 * BQC_DUP_BINS + c), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    block_sync();
    for (uint32_t t = tid; t < 2 * BQC_DUP_BINS; t += DP_FTHREADS) {
        const uint32_t v = s_h[t / BQC_DUP_BINS][t % BQC_DUP_BINS];
        if (v) gadd(out + t, v);
    }
}

// the slots of a table for `capacity` signatures (dup_table.h)
extern "C" uint64_t bqc_dup_slots(uint64_t capacity) { return dp_slots(capacity); }
extern "C" uint64_t bqc_dup_out_words(void) { return 2 * BQC_DUP_BINS + 2; }

// The table, the counter of sets behind it and the sums: empty.
extern "C" void bqc_launch_dup_clear(const DupTable& T, uint64_t* sums, uint32_t n_lanes, uint32_t n_cu, hipStream_t s)
{
    dp_clear(T, n_cu, s);
    (void)hipMemsetAsync(sums, 0, (uint64_t)n_lanes * 5 * 8, s);
}

// Measuring switches: BQC_DUP_COMBINE=0 leaves equal signatures of a wave uncombined, =2 combines them in every wave;
// BQC_DUP_HASH=1 keeps u5's low bits in the slot instead of mixing the whole signature.
extern "C" void bqc_launch_dup(const DevBatch& b, const DupTable& T, uint64_t* sums, uint32_t* err, uint32_t n_lanes, uint32_t n_refs, uint32_t n_cu, hipStream_t s)
{
    if (b.n_reads == 0) return;
    static const uint32_t mode = (env_is("BQC_DUP_COMBINE", '0') ? 1u : 0u) | (env_is("BQC_DUP_COMBINE", '2') ? 4u : 0u) | (env_is("BQC_DUP_HASH", '1') ? 2u : 0u);
    uint32_t per;
    const uint32_t g = share_grid(b.n_reads, n_cu, &per);
    hipLaunchKernelGGL(k_dup, dim3(g), dim3(DP_THREADS), 0, s, b, T, sums, err, n_lanes, n_refs, per, mode);
}

// The finalize pass: the table is read only; out holds bqc_dup_out_words words.
extern "C" void bqc_launch_dup_final(const DupTable& T, uint64_t* out, uint32_t n_cu, hipStream_t s)
{
    const uint64_t C = T.mask + 1u;
    (void)hipMemsetAsync(out, 0, bqc_dup_out_words() * 8, s);
    const uint32_t g = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)n_cu * 8, (C + DP_FTHREADS - 1) / DP_FTHREADS));
    hipLaunchKernelGGL(k_dup_final, dim3(g), dim3(DP_FTHREADS), 0, s, T.slots, C, out);
}
