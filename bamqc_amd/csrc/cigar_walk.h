// cigar_walk.h — what the kernels that walk CIGARs over a share of the batch have in common (k_ibc, k_sac, k_rcv, k_dup, k_wdp; DESIGN
// section 4.2, "walk frame"): the classes of a CIGAR operation, a wave's pass over a long CIGAR, a workgroup's share of the processing
// order, the list of a step's reads for a later path, three sums a read group, and on the host the launch geometry and the reading of
// the measuring switches.  Everything is inline: nothing here is an object of its own.  (sa_find and rc_find stay two functions: one
// bucket lookup for both was measured, and k_sac's and k_rcv's long reads were slower with it.)
#pragma once
#include <algorithm>
#include <cstdlib>
#include "kernels_common.h"

#define WALK_NONE 0xFFFFFFFFu        // no read

// ---- the classes of an operation (BAM: M0 I1 D2 N3 S4 H5 P6 =7 X8) -------------------------------------------------------------------
__device__ __forceinline__ bool cig_match(uint32_t op) { return op == 0u || op == 7u || op == 8u; }
// bases of the read (M, I, S, =, X) and of the genome (M, D, N, =, X) that n of op consume
__device__ __forceinline__ uint32_t cig_qlen(uint32_t op, uint32_t n) { return (op == 0u || op == 1u || op == 4u || op == 7u || op == 8u) ? n : 0u; }
__device__ __forceinline__ uint32_t cig_glen(uint32_t op, uint32_t n) { return (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) ? n : 0u; }

// The sum of v over the wave, exact in 64 bits for v < 2^28 (a CIGAR length): the halves are summed apart, below 2^22 and 2^18.
__device__ __forceinline__ uint64_t wave_sum_split(uint32_t v) { return ((uint64_t)wave_sum(v >> 16) << 16) + wave_sum(v & 0xFFFFu); }

// ---- a wave's walk over a long CIGAR -------------------------------------------------------------------------------------------------
// A pass is 64 operations, one per lane, and the next 64 words are loaded before the pass is worked on.  The stored index jj of a
// lane's operation is the carry of the passes before plus the exclusive prefix of the pass's read-consuming lengths; with GENOME its
// genome position gg comes the same way from pos and the genome-consuming lengths.  THE SCANS ARE 64-BIT, not saturated: a length has
// 28 bits, so its low 16 and its high 12 bits are scanned apart by wave_scan_incl (sums below 2^22 and 2^18) and put together as
// hi << 16 + lo; the carries are 64-bit scalars (at most 65 535 x 2^28 < 2^44).  Every comparison of a rule is made on those exact
// values.  Once the carry of j has reached L no later operation holds a base of the read, and advance() ends the walk.
//     CigWalk<true> cw;
//     cw.start(cg, coff, nc, L, pos);
//     for (uint32_t p0 = 0; p0 < nc; p0 += WAVE) { cw.pass(p0, op, n, jj, gg); ...; if (!cw.advance()) break; }
// The loop and its counter are the caller's, an ordinary for with its test at the top and the exit on the carry inside: with the
// counter in here k_rcv took two registers more and lost a wave of occupancy, and in a loop rotated around one flag the compiler
// waited for the word loaded ahead as soon as it had asked for it.
// The body runs with all 64 lanes: a lane behind the CIGAR's end has op 0 and n 0 (an M of no bases) and pass() returns false for it.
// load() alone is the pass without the scans (k_dup).  k_ibc and k_wdp walk with it; k_sac and k_rcv keep the same pass written out
// in their files, because their long reads measured 1 to 3 % slower through this type (profiles/walk_frame_compare.txt).
template <bool GENOME>
struct CigWalk {
    const gmem_u32* cg;
    uint32_t coff, nc, L, wd_n;
    int64_t pos;
    uint64_t cj, cgp;                // the carries: bases of the read and of the genome in front of this pass
    uint32_t qlo, qhi, glo, ghi;     // this pass's inclusive scans

    __device__ __forceinline__ void start(const gmem_u32* cg_, uint32_t coff_, uint32_t nc_, uint32_t L_ = 0u, int64_t pos_ = 0)
    {
        cg = cg_; coff = coff_; nc = nc_; L = L_; pos = pos_;
        cj = 0; cgp = 0;
        const uint32_t ln = (uint32_t)lane_id();
        wd_n = ln < nc ? cg[(uint64_t)coff + ln] : 0u;
    }
    // this lane's operation of the pass from operation p0 on (false: behind the CIGAR's end)
    __device__ __forceinline__ bool load(uint32_t p0, uint32_t& op, uint32_t& n)
    {
        const uint32_t ln = (uint32_t)lane_id(), wd = wd_n;
        const uint32_t kn = p0 + WAVE + ln; // (nc <= 65 535: no wrap)
        wd_n = kn < nc ? cg[(uint64_t)coff + kn] : 0u;
        op = wd & 15u; n = wd >> 4;
        return p0 + ln < nc;
    }
    __device__ __forceinline__ bool pass(uint32_t p0, uint32_t& op, uint32_t& n, uint64_t& jj, int64_t& gg)
    {
        const bool valid = load(p0, op, n);
        const uint32_t q = cig_qlen(op, n), gl = GENOME ? cig_glen(op, n) : 0u;
        qlo = wave_scan_incl(q & 0xFFFFu); qhi = wave_scan_incl(q >> 16);
        if (GENOME) { glo = wave_scan_incl(gl & 0xFFFFu); ghi = wave_scan_incl(gl >> 16); }
        jj = cj + (((uint64_t)qhi << 16) + qlo) - q;
        gg = GENOME ? pos + (int64_t)(cgp + (((uint64_t)ghi << 16) + glo) - gl) : pos;
        return valid;
    }
    // the carries from lane 63; false when the read is used up
    __device__ __forceinline__ bool advance()
    {
        cj += ((uint64_t)__builtin_amdgcn_readlane(qhi, 63) << 16) + __builtin_amdgcn_readlane(qlo, 63);
        if (GENOME) cgp += ((uint64_t)__builtin_amdgcn_readlane(ghi, 63) << 16) + __builtin_amdgcn_readlane(glo, 63);
        return cj < L;
    }
};

// ---- a workgroup's share of the processing order -------------------------------------------------------------------------------------
// Workgroup x takes the reads [x per, (x + 1) per) of the order (false: none), STEP at a time, thread t of a step the step's read t.
__device__ __forceinline__ bool wg_share(uint32_t n_reads, uint32_t per, uint32_t& begin, uint32_t& end)
{
    const uint64_t begin64 = (uint64_t)blockIdx.x * per;
    if (begin64 >= n_reads) return false;
    begin = (uint32_t)begin64;
    end = (uint32_t)min((uint64_t)n_reads, begin64 + per);
    return true;
}
// read i of the processing order (WALK_NONE: behind the share's end, or no read of the batch)
__device__ __forceinline__ uint32_t batch_read(const DevBatch& b, uint64_t i, uint32_t end)
{
    if (i >= end) return WALK_NONE;
    const uint32_t r = b.order ? b.order[i] : (uint32_t)i;
    return r < b.n_reads ? r : WALK_NONE;
}
// the step at `base` is the share's last (what ends the loop over the steps, not its own test: base + STEP may wrap)
__device__ __forceinline__ bool last_step(uint32_t base, uint32_t end, uint32_t STEP) { return end - base <= STEP; }

// ---- the reads a step lists for a later path -----------------------------------------------------------------------------------------
// The lists are double-buffered by the step's parity and their counters are three, zeroed a step after their use: a counter is read
// last in front of the step's barrier and added to again only behind the next one.  That is what makes one barrier a step enough.
struct StepTurn {
    uint32_t par = 0, cnt = 0;       // the step's buffer and its counter
    __device__ __forceinline__ void next() { par ^= 1u; cnt = cnt == 2u ? 0u : cnt + 1u; }
    __device__ __forceinline__ uint32_t prev() const { return cnt ? cnt - 1u : 2u; } // the step before's counter
};
// In LDS.  LISTS lists of one step share the payload: a thread is on one of them at most.
template <uint32_t STEP, uint32_t LISTS = 1>
struct StepList {
    uint32_t who[LISTS][2][STEP];    // the listed reads of a step: the threads that fetched them
    uint32_t r[2][STEP];             // their reads, by thread
    uint32_t n[3][LISTS];            // [step mod 3] listed reads

    __device__ __forceinline__ void zero() // (the caller's barrier follows)
    {
        if (threadIdx.x < 3u * LISTS) n[threadIdx.x / LISTS][threadIdx.x % LISTS] = 0;
    }
    // the WHOLE WAVE calls: the lanes with pred are ranked by ballot, one LDS atomic a wave and list
    __device__ __forceinline__ void push(const StepTurn& t, bool pred, uint32_t read, uint32_t list = 0u)
    {
        const uint32_t ln = (uint32_t)lane_id();
#pragma unroll
        for (uint32_t l = 0; l < LISTS; ++l) {
            const bool mine = pred && (LISTS == 1u || list == l);
            const uint64_t bl = __ballot(mine);
            if (bl) {
                uint32_t at = 0;
                if (ln == 0) at = atomicAdd(&n[t.cnt][l], (uint32_t)__popcll((unsigned long long)bl));
                at = __builtin_amdgcn_readfirstlane(at);
                if (mine) who[l][t.par][at + (uint32_t)__popcll((unsigned long long)(bl & ((1ull << ln) - 1ull)))] = threadIdx.x;
            }
        }
        if (pred) r[t.par][threadIdx.x] = read;
    }
    // the step's barrier; behind it the lists are whole and the step before's counters are cleared.  Returns list 0's reads.
    __device__ __forceinline__ uint32_t close(const StepTurn& t)
    {
        block_sync();
        if (threadIdx.x < LISTS) n[t.prev()][threadIdx.x] = 0;
        return n[t.cnt][0];
    }
    __device__ __forceinline__ uint32_t count(const StepTurn& t, uint32_t l) const { return n[t.cnt][l]; }
    __device__ __forceinline__ uint32_t thread(const StepTurn& t, uint32_t e, uint32_t l = 0u) const { return who[l][t.par][e]; }
    __device__ __forceinline__ uint32_t read(const StepTurn& t, uint32_t thr) const { return r[t.par][thr]; }
};

// ---- three sums a read group ---------------------------------------------------------------------------------------------------------
// Never one atomic a read: a wave sums over its lanes by read group and its leader hands the sums in here.  The read groups below
// ETA_LANES have a copy in LDS, which the workgroup adds to memory once, at its end; the others go to memory at once.  The sums are the
// first three words of a read group's lane_words.
#define ETA_LANES 64
typedef unsigned long long (*EtaTab)[3];
__device__ __forceinline__ void eta_zero(EtaTab s_eta) // (the caller's barrier follows)
{
    if (threadIdx.x < ETA_LANES * 3) s_eta[threadIdx.x / 3][threadIdx.x % 3] = 0;
}
__device__ __forceinline__ void eta_add(EtaTab s_eta, uint64_t* state, uint64_t lane_words, uint32_t gl, uint64_t a, uint64_t b, uint64_t c)
{
    if (gl < ETA_LANES) {
        if (a) atomicAdd(&s_eta[gl][0], (unsigned long long)a);
        if (b) atomicAdd(&s_eta[gl][1], (unsigned long long)b);
        if (c) atomicAdd(&s_eta[gl][2], (unsigned long long)c);
    } else {
        uint64_t* h = state + (uint64_t)gl * lane_words; // (gl < n_lanes: an examined read's)
        if (a) gadd(h, a);
        if (b) gadd(h + 1, b);
        if (c) gadd(h + 2, c);
    }
}
__device__ __forceinline__ void eta_flush(EtaTab s_eta, uint64_t* state, uint64_t lane_words, uint32_t n_lanes) // (behind the caller's barrier)
{
    if (threadIdx.x < ETA_LANES * 3) {
        const uint32_t l = threadIdx.x / 3, w = threadIdx.x % 3;
        const unsigned long long v = s_eta[l][w];
        if (v && l < n_lanes) gadd(state + (uint64_t)l * lane_words + w, v);
    }
}

// ---- the host's side -----------------------------------------------------------------------------------------------------------------
// Workgroups of a kernel that shares the batch's reads out: about one per CU, none with fewer than 256 reads unless it is the only
// one; each takes `per` consecutive reads of the processing order.
inline uint32_t share_grid(uint32_t n_reads, uint32_t n_cu, uint32_t* per)
{
    const uint32_t g = std::max(1u, std::min(n_cu, (uint32_t)(((uint64_t)n_reads + 255) / 256)));
    *per = (uint32_t)(((uint64_t)n_reads + g - 1) / g);
    return g;
}
// A measuring switch of the environment: a number of lo .. hi (anything else: dflt); is it the one character c
inline uint32_t env_uint(const char* name, long lo, long hi, uint32_t dflt)
{
    const char* e = getenv(name);
    const long v = e && *e ? strtol(e, nullptr, 10) : lo - 1;
    return v >= lo && v <= hi ? (uint32_t)v : dflt;
}
inline bool env_is(const char* name, char c)
{
    const char* e = getenv(name);
    return e && e[0] == c && !e[1];
}
