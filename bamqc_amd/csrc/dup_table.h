// dup_table.h — the exact hash table in device memory that counts sets of equal two-word keys: k_dup.hip's (duplicate sets by alignment
// signature) and k_ovr.hip's (sets of equal read sequences).  Everything is inline or has internal linkage: nothing here is an object of
// its own, and either file has its own copy of the clearing kernel.
//
// The table.  C slots (a power of two, at least twice the capacity in keys) of DupSlot {k0, k1, count}, open addressing with linear
// probing; an empty key word is all ones — the user's layout keeps both of its words off that value.  Every access to a key word or a
// count while keys are inserted is an 8-byte agent-scope atomic: nothing is fenced, and no L1 can serve a stale key.
// The insert never waits for another thread.  At a slot: (1) k0 is loaded, and if empty claimed by a compare-and-swap; (2) if the
// slot's k0 is now this key's, the same for k1; (3) if k1 is this key's too the slot is the key's, and its count is added to — the
// thread whose compare-and-swap of k1 succeeded has made a new set; (4) otherwise both words are set, stay as they are for good, and
// belong to another key: the next slot.  k0 may be claimed by one thread and k1 by another with the same k0: the slot then holds the
// second thread's key and the first moves on.  Every thread of one key sees the same immutable words at every slot of its probe
// sequence, so all of them end in the same slot: no two keys share a set, no key has two.
// The bound.  The user counts its new sets (per workgroup and step in LDS) and adds them to one word behind the table, n_sets.  A probe
// sequence looks at that word every DP_CHECK slots and gives up when it has passed the capacity; it also gives up after C slots.
#pragma once
#include <algorithm>
#include "kernels_common.h"

#define DP_CHECK 64                  // slots of a probe sequence between two looks at the counter of sets

typedef unsigned long long dp_u64;
__device__ __forceinline__ dp_u64 dp_load(const uint64_t* p) { return __hip_atomic_load((const gmem_u64*)(uintptr_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// compare-and-swap of an empty word with `mine`: what the word holds afterwards; won: this thread's swap took place
__device__ __forceinline__ dp_u64 dp_claim(uint64_t* p, dp_u64 mine, bool& won)
{
    dp_u64 seen = BQC_DUP_EMPTY;
    won = __hip_atomic_compare_exchange_strong((gmem_u64*)(uintptr_t)p, &seen, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return won ? mine : seen;
}

__device__ __forceinline__ uint64_t dp_mix(uint64_t x)
{
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return x;
}
__device__ __forceinline__ uint64_t dp_slot(uint64_t k0, uint64_t k1, uint64_t mask, uint32_t mode)
{
    if (!(mode & 2u)) return dp_mix(k0 ^ dp_mix(k1)) & mask;
    return ((dp_mix((k0 >> 6) ^ dp_mix(k1)) << 6) | (k0 & 63u)) & mask; // (k_dup's measuring switch: k1 whole and k0 without its low 6 bits)
}

// n reads of one key.  Returns 1 when the set is new, 0 when it was there or the sequence gave up (`over`).
__device__ __forceinline__ uint32_t dp_insert(const DupTable& T, uint64_t k0, uint64_t k1, uint64_t n, uint32_t mode, bool& over)
{
    uint64_t s = dp_slot(k0, k1, T.mask, mode);
    for (uint64_t probes = 0; probes <= T.mask; ++probes, s = (s + 1u) & T.mask) {
        if ((probes & (DP_CHECK - 1u)) == DP_CHECK - 1u && dp_load(T.n_sets) > T.capacity) break;
        DupSlot* sl = T.slots + s;
        bool won = false;
        dp_u64 a = dp_load(&sl->k0);
        if (a == BQC_DUP_EMPTY) a = dp_claim(&sl->k0, k0, won);
        if (a != k0) continue;
        won = false;
        dp_u64 b = dp_load(&sl->k1);
        if (b == BQC_DUP_EMPTY) b = dp_claim(&sl->k1, k1, won);
        if (b != k1) continue;
        gadd(&sl->count, n);
        return won ? 1u : 0u;
    }
    over = true;
    return 0;
}

static __global__ void k_dup_clear(DupSlot* slots, uint64_t C)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
    uint64_t* w = (uint64_t*)slots;
    for (uint64_t x = i; x < 3u * C; x += step) w[x] = x % 3u == 2u ? 0ull : BQC_DUP_EMPTY;
}

// the slots of a table for `capacity` keys: the smallest power of two >= 2 capacity (capacity <= 2^31)
inline uint64_t dp_slots(uint64_t capacity)
{
    uint64_t C = 32;
    while (C < 2 * capacity) C <<= 1;
    return C;
}
// The table and the counter of sets behind it: empty.
static inline void dp_clear(const DupTable& T, uint32_t n_cu, hipStream_t s)
{
    const uint64_t C = T.mask + 1u;
    const uint32_t g = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)n_cu * 8, (3 * C + 1023) / 1024));
    hipLaunchKernelGGL(k_dup_clear, dim3(g), dim3(1024), 0, s, T.slots, C);
    (void)hipMemsetAsync(T.n_sets, 0, 8, s);
}
// the workgroups of a finalize pass over the C slots, `threads` a workgroup
inline uint32_t dp_scan_grid(uint64_t C, uint32_t threads, uint32_t n_cu)
{
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)n_cu * 8, (C + threads - 1) / threads));
}
