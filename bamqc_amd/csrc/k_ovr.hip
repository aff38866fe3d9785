// k_ovr.hip — overrepresented sequences and duplication by sequence (--overrepresented; the rule: include/bamqc.h):
// every examined read has a key — its first n = min(l_seq, K) bases AS SEQUENCED, n and the mate — two reads with equal keys are in one
// set, and the sets are counted EXACTLY in dup_table.h's hash table in device memory.  A read with a base other than A, C, G, T among
// the n is skipped.  An optional module beside k_dup: its launches and its memory exist only when bqc_enable_overrepresented has been
// called.  No quality, CIGAR, contig or genome is read.  The module's state is NOT part of the flat state vector.
//
// The key.  2 bits a base (A 0, C 1, G 2, T 3), sequenced base 0 lowest, 28 bases a word: k0 = bases 0..27 | n << 56 | mate << 62,
// k1 = bases 28..55; the bits of bases at or behind n are zero.  Bit 63 of k0 and the top byte of k1 are never set: neither word can
// be the table's empty mark (all ones), whatever the bases — 28 T are 56 set bits.
//
// k_ovr, per batch.  The share-out frame of cigar_walk.h: about one workgroup per CU, OV_WAVES waves; a workgroup takes a contiguous
// share of the batch's processing order, OV_STEP reads at a time, thread t of a step fetching the columns of the step's read t (those
// of the next step before this one is inserted).
// A THREAD A READ.  The n bases are stored bases 0..n-1 of a forward read and L-n..L-1 of a reverse read: at most 28 bytes, 29 when a
// reverse read's window starts in a byte's low nibble, starting at any byte.  The thread takes the aligned dwords that hold one of
// those bytes (at most 8; every one holds a byte of the read, so the loads stay inside the payload), shifts them to the window's first
// byte (alignbyte) and packs them with ad_pack8: 128 bits of codes and 64 bits of "is A, C, G or T".  An odd start shifts both by a
// base; only the n lowest validity bits are asked, and the codes are cut to n bases: the pad nibble of an odd length, the bytes of the
// next read and a dword that was not loaded never reach a key.  A reverse read's window is turned (bit reversal, the bits of a pair
// swapped back), moved down by 64 - n bases and complemented (the complement of a code c is 3 - c, its bitwise inverse).
// (A few lanes a read — a dword a lane through the packer, combined by shuffles, as k_adp shares a read out — was NOT built: a key needs
// 8 dwords where k_adp's search needs up to 64 a read, and the kernel is bound by the table's atomics, not by the packer)
// Equal keys of a wave are combined by ballots before the table is touched, one insert with their number — in the waves where some
// lane's key is that of one of the two lanes in front of it (BQC_OVR_COMBINE=0: never; =2: in every wave).  A hot sequence arrives side
// by side, and with the mates of a pair interleaved every other read is of the same mate: the lane beside alone (k_dup's test) never
// met an equal key on such input (measured: DESIGN 4.2n).
// New sets are counted per workgroup and step in LDS (two counters by the step's parity: one is added to in front of the step's
// barrier and flushed behind it) and added to the word behind the table once a step; dup_table.h says what the probe sequences make
// of it.  More keys than the capacity set BQC_DEVERR_OVR in the batch's error record: the stream fails with BQC_ERR_RANGE.
// The four sums of a read group (examined and skipped by mate) are ballots by read group, added to the workgroup's LDS copy and once,
// at the workgroup's end, to memory.
//
// k_ovr_final, at bqc_finalize only: one pass over the C slots, which it only reads: the sets by mate and size into LDS histograms
// (one add a bin and workgroup to memory), the largest set by a maximum per wave, and every set of mate m with at least thr[m] reads
// — the host has the thresholds from the sums — appended to a list, key words and count: a wave's hits take their places with ONE add
// to the list's counter.  The list has room for every set that can reach the threshold (include/bamqc.h: the derived bound); a hit
// behind its end is not written and sets BQC_DEVERR_INTERNAL.
#include "cigar_walk.h"
#include "dup_table.h" // the table: slot, claim, insert, clear (also k_dup.hip's)

#define OV_THREADS 1024
#define OV_WAVES (OV_THREADS / WAVE)
#define OV_STEP OV_THREADS
#define OV_LANES 256                 // read groups (the lane column is a byte)
#define OV_NONE WALK_NONE
#define OV_FTHREADS 256

// the 32 bases of a word in reverse order
__device__ __forceinline__ uint64_t ov_turn(uint64_t x)
{
    x = __brevll(x);
    return ((x & 0xAAAAAAAAAAAAAAAAull) >> 1) | ((x & 0x5555555555555555ull) << 1);
}
// (hi : lo) >> s, 0 <= s < 128
__device__ __forceinline__ void ov_shr(uint64_t& lo, uint64_t& hi, uint32_t s)
{
    if (s >= 64u) { lo = hi >> (s - 64u); hi = 0; }
    else if (s) { lo = (lo >> s) | (hi << (64u - s)); hi >>= s; }
}

// The key of a read of L > 0 bases whose bytes start at seq + soff (false: one of its n bases is not A, C, G or T).  20 <= K <= 56.
__device__ __forceinline__ bool ov_key(const uint8_t* __restrict__ seq, uint32_t soff, uint32_t L, bool rev, uint32_t mate, uint32_t K, uint64_t& k0, uint64_t& k1)
{
    const uint32_t n = min(L, K), s = rev ? L - n : 0u;    // the window: stored bases s .. s + n - 1
    const uint32_t odd = s & 1u, nb = (odd + n + 1u) >> 1; // its bytes (at most 29), every one a byte of the read
    const uintptr_t p = (uintptr_t)(seq + soff) + (s >> 1);
    const uint32_t sh = (uint32_t)p & 3u, span = sh + nb;  // the bytes from the aligned dword of p on that are needed (at most 32)
    const gmem_u32* a = (const gmem_u32*)(p & ~(uintptr_t)3); // (global, said so: through the integer the compiler sees a flat pointer)
    uint32_t d[9];
    d[0] = a[0];
#pragma unroll
    for (uint32_t i = 1; i < 8; ++i) d[i] = 4u * i < span ? a[i] : 0u;
    d[8] = 0u;
    uint64_t lo = 0, hi = 0, valid = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
        uint32_t c, v;
        ad_pack8(__builtin_amdgcn_alignbyte(d[i + 1], d[i], sh), c, v);
        if (i < 4) lo |= (uint64_t)c << (16 * i);
        else hi |= (uint64_t)c << (16 * (i - 4));
        valid |= (uint64_t)v << (8 * i);
    }
    if (odd) { ov_shr(lo, hi, 2); valid >>= 1; }
    const uint64_t vm = (1ull << n) - 1ull;                // (n <= 56)
    if ((valid & vm) != vm) return false;
    if (rev) { // sequenced base i is the complement of the window's base n - 1 - i
        const uint64_t t = ov_turn(hi);
        hi = ov_turn(lo); lo = t;
        ov_shr(lo, hi, 2u * (64u - n));
        lo = ~lo; hi = ~hi;
    }
    if (2u * n >= 64u) hi &= (1ull << (2u * n - 64u)) - 1ull; // the n bases and nothing behind them
    else { hi = 0; lo &= (1ull << (2u * n)) - 1ull; }
    k0 = (lo & 0x00FFFFFFFFFFFFFFull) | (uint64_t)n << 56 | (uint64_t)mate << 62;
    k1 = (lo >> 56) | (hi << 8);
    return true;
}

// Read i of the processing order: where its bases start, its length, mate and strand, and its read group (OV_NONE: not examined)
struct OvRead { uint32_t soff, L, info, lane; }; // info: mate | reverse << 1
__device__ __forceinline__ OvRead ov_fetch(const DevBatch& b, uint64_t i, uint32_t end, uint32_t n_lanes)
{
    OvRead o{0u, 0u, 0u, OV_NONE};
    const uint32_t r = batch_read(b, i, end);
    if (r == WALK_NONE) return o;
    const uint32_t f = b.flag[r], L = b.l_seq[r], g = b.lane[r];
    if ((f & 0x900u) || !(f & 0xC0u) || !L || g >= n_lanes) return o;
    o.soff = b.seq_off[r];
    o.L = L;
    o.info = ((f & 0x40u) ? 0u : 1u) | ((f >> 4) & 1u) << 1;
    o.lane = g;
    return o;
}

__global__ __launch_bounds__(OV_THREADS) void k_ovr(DevBatch b, DupTable T, uint64_t* __restrict__ sums, uint32_t* __restrict__ err, uint32_t n_lanes, uint32_t K, uint32_t per, uint32_t mode)
{
    __shared__ uint32_t s_new[2];                           // [step's parity] new sets
    __shared__ uint32_t s_full;                             // the table went over its capacity in an earlier batch
    __shared__ unsigned long long s_sum[OV_LANES][4];       // the workgroup's sums by read group: examined by mate, skipped by mate
    if (b.desc->fatal) return;
    if (threadIdx.x == 0) s_full = dp_load(T.n_sets) > T.capacity ? 1u : 0u;
    block_sync();
    if (s_full) return;                                     // (the stream has failed; one thread looks, so the whole workgroup leaves or stays)
    const uint32_t tid = threadIdx.x, ln = lane_id();
    uint32_t begin, end;
    if (!wg_share(b.n_reads, per, begin, end)) return;
    if (tid < 2) s_new[tid] = 0;
    for (uint32_t t = tid; t < OV_LANES * 4; t += OV_THREADS) s_sum[t / 4][t % 4] = 0;
    block_sync();
    bool over = false;
    uint32_t par = 0;
    OvRead nx = ov_fetch(b, (uint64_t)begin + tid, end, n_lanes);
    for (uint32_t base = begin; base < end; base += OV_STEP, par ^= 1u) {
        const OvRead me = nx;
        if (!last_step(base, end, OV_STEP)) nx = ov_fetch(b, (uint64_t)base + OV_STEP + tid, end, n_lanes); // (in flight while this step is inserted)
        const bool ex = me.lane != OV_NONE;
        const uint32_t mate = me.info & 1u;
        uint64_t k0 = 0, k1 = 0, n = 1;
        bool ins = ex && ov_key(b.seq, me.soff, me.L, (me.info >> 1) & 1u, mate, K, k0, k1);
        // the sums, by read group
        {
            uint64_t m = __ballot(ex);
            while (m) {
                const int leader = __ffsll((unsigned long long)m) - 1;
                const uint32_t gl = __builtin_amdgcn_readlane(me.lane, leader);
                const bool same = ex && me.lane == gl;
                const uint64_t sm = __ballot(same);
                const uint32_t e0 = (uint32_t)__popcll((unsigned long long)__ballot(same && mate == 0u)), e1 = (uint32_t)__popcll((unsigned long long)sm) - e0;
                const uint32_t q0 = (uint32_t)__popcll((unsigned long long)__ballot(same && !ins && mate == 0u)), q1 = (uint32_t)__popcll((unsigned long long)__ballot(same && !ins && mate == 1u));
                if ((int)ln == leader) {
                    if (e0) atomicAdd(&s_sum[gl][0], (unsigned long long)e0);
                    if (e1) atomicAdd(&s_sum[gl][1], (unsigned long long)e1);
                    if (q0) atomicAdd(&s_sum[gl][2], (unsigned long long)q0);
                    if (q1) atomicAdd(&s_sum[gl][3], (unsigned long long)q1);
                }
                m &= ~sm;
            }
        }
        // equal keys of the wave: the first lane of each takes them all — where a lane's key is that of one of the two lanes in front of it
        // (the mate is part of the key, and the mates of a pair lie side by side in unaligned and name-sorted files: first, second, first ...)
        const uint32_t digest = ins ? (uint32_t)k0 ^ (uint32_t)(k0 >> 32) ^ (uint32_t)k1 * 0x9E3779B1u ^ (uint32_t)(k1 >> 32) : ln;
        const bool beside = ins && ((ln > 0 && (uint32_t)__shfl_up((int)digest, 1) == digest) || (ln > 1 && (uint32_t)__shfl_up((int)digest, 2) == digest));
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
        if (ins) fresh = dp_insert(T, k0, k1, n, mode & ~2u, over);
        {
            const uint64_t fm = __ballot(fresh != 0u);
            if (fm && ln == 0) atomicAdd(&s_new[par], (uint32_t)__popcll((unsigned long long)fm));
        }
        block_sync();
        if (tid == 0) { // this step's new sets: whole behind the barrier, and the counter is added to again only behind the next one
            const uint32_t v = s_new[par];
            if (v) gadd(T.n_sets, v);
            s_new[par] = 0;
        }
        if (last_step(base, end, OV_STEP)) break;
    }
    if (over) atomicOr(err, BQC_DEVERR_OVR);
    block_sync();
    for (uint32_t t = tid; t < OV_LANES * 4; t += OV_THREADS) {
        const unsigned long long v = s_sum[t / 4][t % 4];
        if (v) gadd(sums + t, v); // (a read group with a sum is below n_lanes)
    }
    if (tid == 0 && dp_load(T.n_sets) > T.capacity) atomicOr(err, BQC_DEVERR_OVR); // (every step's sets are in the word: the last workgroup sees them all)
}

// ---- finalize ----------------------------------------------------------------------------------------------------------------------
// out: [2 mates][BQC_DUP_BINS] sets by size, the two largest sets, the list's counter, a spare word, then the list [list_cap][3: k0,
// k1, count]; the first BQC_OVR_HEAD words zero before the launch.
__global__ __launch_bounds__(OV_FTHREADS) void k_ovr_final(const DupSlot* __restrict__ slots, uint64_t C, uint64_t thr0, uint64_t thr1, uint64_t* __restrict__ out, uint64_t list_cap, uint32_t* __restrict__ err)
{
    __shared__ uint32_t s_h[2][BQC_DUP_BINS]; // (a workgroup takes fewer than 2^32 slots)
    const uint32_t tid = threadIdx.x, ln = lane_id();
    for (uint32_t t = tid; t < 2 * BQC_DUP_BINS; t += OV_FTHREADS) s_h[t / BQC_DUP_BINS][t % BQC_DUP_BINS] = 0;
    block_sync();
    uint64_t big[2] = {0, 0};
    bool behind = false;
    const uint64_t step = (uint64_t)gridDim.x * OV_FTHREADS;
    for (uint64_t x0 = (uint64_t)blockIdx.x * OV_FTHREADS; x0 < C; x0 += step) { // (the whole wave makes every turn: the ballots below)
        const uint64_t x = x0 + tid;
        uint64_t k0 = BQC_DUP_EMPTY, k1 = 0, n = 0;
        if (x < C) {
            k0 = slots[x].k0;
            if (k0 != BQC_DUP_EMPTY) { k1 = slots[x].k1; n = slots[x].count; }
        }
        const bool live = k0 != BQC_DUP_EMPTY && n; // (n is never 0: the add follows the claim of k1; a bin below the first does not exist)
        const uint32_t mate = (uint32_t)(k0 >> 62) & 1u;
        if (live) {
            atomicAdd(&s_h[mate][(n < BQC_DUP_BINS ? (uint32_t)n : (uint32_t)BQC_DUP_BINS) - 1u], 1u);
            big[mate] = n > big[mate] ? n : big[mate];
        }
        const bool hit = live && n >= (mate ? thr1 : thr0);
        const uint64_t hm = __ballot(hit);
        if (hm) {
            dp_u64 at = 0;
            if (ln == 0) at = __hip_atomic_fetch_add((gmem_u64*)(uintptr_t)(out + BQC_OVR_HEAD - 2), (dp_u64)__popcll((unsigned long long)hm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t first = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)at) | (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(at >> 32)) << 32;
            if (hit) {
                const uint64_t e = first + (uint64_t)__popcll((unsigned long long)(hm & ((1ull << ln) - 1ull)));
                if (e < list_cap) { uint64_t* w = out + BQC_OVR_HEAD + 3u * e; w[0] = k0; w[1] = k1; w[2] = n; }
                else behind = true;
            }
        }
    }
    if (behind) atomicOr(err, BQC_DEVERR_INTERNAL);
#pragma unroll
    for (uint32_t c = 0; c < 2; ++c) {
        uint64_t v = big[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t t = (uint64_t)__shfl_xor((unsigned long long)v, o);
            v = t > v ? t : v;
        }
        if (ln == 0 && v) __hip_atomic_fetch_max((gmem_u64*)(uintptr_t)(out + 2 * BQC_DUP_BINS + c), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    block_sync();
    for (uint32_t t = tid; t < 2 * BQC_DUP_BINS; t += OV_FTHREADS) {
        const uint32_t v = s_h[t / BQC_DUP_BINS][t % BQC_DUP_BINS];
        if (v) gadd(out + t, v);
    }
}

// the words of k_ovr_final's products for a list of list_cap sets
extern "C" uint64_t bqc_ovr_out_words(uint64_t list_cap) { return BQC_OVR_HEAD + 3 * list_cap; }

// The table, the counter of sets behind it and the sums: empty.
extern "C" void bqc_launch_ovr_clear(const DupTable& T, uint64_t* sums, uint32_t n_lanes, uint32_t n_cu, hipStream_t s)
{
    dp_clear(T, n_cu, s);
    (void)hipMemsetAsync(sums, 0, (uint64_t)n_lanes * 4 * 8, s);
}

// Measuring switch: BQC_OVR_COMBINE=0 leaves equal keys of a wave uncombined, =2 combines them in every wave.
extern "C" void bqc_launch_ovr(const DevBatch& b, const DupTable& T, uint64_t* sums, uint32_t* err, uint32_t n_lanes, uint32_t K, uint32_t n_cu, hipStream_t s)
{
    if (b.n_reads == 0) return;
    static const uint32_t mode = (env_is("BQC_OVR_COMBINE", '0') ? 1u : 0u) | (env_is("BQC_OVR_COMBINE", '2') ? 4u : 0u);
    uint32_t per;
    const uint32_t g = share_grid(b.n_reads, n_cu, &per);
    hipLaunchKernelGGL(k_ovr, dim3(g), dim3(OV_THREADS), 0, s, b, T, sums, err, n_lanes, K, per, mode);
}

// The finalize pass: the table is read only; out holds bqc_ovr_out_words(list_cap) words, thr the two thresholds by mate.
extern "C" void bqc_launch_ovr_final(const DupTable& T, const uint64_t* thr, uint64_t* out, uint64_t list_cap, uint32_t* err, uint32_t n_cu, hipStream_t s)
{
    const uint64_t C = T.mask + 1u;
    (void)hipMemsetAsync(out, 0, BQC_OVR_HEAD * 8, s);
    hipLaunchKernelGGL(k_ovr_final, dim3(dp_scan_grid(C, OV_FTHREADS, n_cu)), dim3(OV_FTHREADS), 0, s, T.slots, C, thr[0], thr[1], out, list_cap, err);
}
