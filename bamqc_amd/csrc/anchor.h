// anchor.h — the order-dependent part of OverallNumbers::coverage (OverallNumbers.hpp:84-110) ON THE CARD (k_anchor.hip), for
// batches whose fixed columns already live in device memory (the reader on the card, gpu_bam.hip): the columns then never come back
// to the host, which only sees a summary of a few hundred bytes and the list of reads at which the window index changes.  Also the
// two functions that ARE the rule — which reads enter coverage() and what one of them does to a read group's windows — for every
// place that applies it, on the host and on the card.
#pragma once
#include <stdint.h>

#include "../../include/bamqc.h"
#include "device_types.h"

// THE RULE, stated once for the host's pass (bqc_pipeline.cpp) and the card's kernels (k_anchor.hip); plain C++, no device pass needed.
#if defined(__HIP__) || defined(__HIPCC__)
#define AN_RULE __host__ __device__ __forceinline__
#else
#define AN_RULE inline
#endif
// which reads enter coverage(): a primary record with a first / last flag, mapped, not a duplicate, on a main chromosome, of a read
// group the context has (bamqualcheck.cpp:318-327,392,430-433)
AN_RULE bool an_is_candidate(uint32_t flag, int32_t rid, uint32_t n_refs, const uint8_t* main_chrom, uint32_t lane, uint32_t n_lanes)
{
    return !((flag & 0xD04u) || !(flag & 0xC0u) || (uint32_t)rid >= n_refs || !main_chrom[rid] || lane >= n_lanes);
}
// one read at beginPos b of chromosome rid enters coverage() (OverallNumbers.hpp:84-110): moves {first, id, shift} and adds the windows
// flushed to `win` (a reset flushes two, a slide one); returns the read's position in the two live windows, 0 .. 2000.  Unsigned
// 32-bit arithmetic as the reference's: a read in front of `shift` resets.
template <class Win>
AN_RULE uint32_t an_step(bool& first, int32_t& id, uint32_t& shift, Win& win, int32_t rid, uint32_t b)
{
    if (first) { first = false; id = rid; shift = b; }
    if (id != rid || b - shift > 2u * BQC_VSIZE) { id = rid; shift = b; win += 2; }
    uint32_t p = b - shift;
    if (p > BQC_VSIZE && p < 2u * BQC_VSIZE) { shift += BQC_VSIZE; p -= BQC_VSIZE; win += 1; }
    return p;
}

// the window state machine of one read group between two reads (host mirror: LaneCov, bqc_ctx.h)
struct AnchorState {
    uint32_t first;   // no read has entered coverage() yet
    int32_t id;       // chromosome of the live windows
    uint32_t shift;   // position of the first live window's first base
    uint32_t pad;
    uint64_t win;     // absolute index (flush order) of the first live window
    // A shard that starts inside the stream (bqc_options.shard_tail): its reads are SET ASIDE (BQC_COV_PENDING) up to the first one
    // that resets the windows whatever their state — another chromosome, or more than 2000 positions from the read before
    // (bqc_pipeline.cpp: host_pass) —, from which on the shard runs as a stream of its own.
    uint32_t pending;  // still setting aside
    uint32_t has_prev; // a read has been seen (prev_rid / prev_bp are the last one's)
    int32_t prev_rid;
    uint32_t prev_bp;
};

// what the host needs from a batch besides the anchors themselves: the batch's facts here, and behind it in the same buffer one
// AnchorLane per read group (n_lanes of them)
struct AnchorSummary {
    uint32_t n_cand;        // reads that enter coverage()
    uint32_t n_breaks;      // candidates that are not < 1000 positions behind the candidate before them on the same chromosome
    uint32_t flags;         // AN_FLAG_*
    uint32_t n_slow;        // reads of the generic path (longer than BQC_FAST_MAXLEN, or every read with no_fast)
    uint32_t max_len_slow;
    uint32_t n_noqual;      // primary first / last records without qualities (check_read_len's message, QualityCheck.hpp:70-79)
    int32_t rid_min, rid_max; // range of the reference ids in [0, n_refs) the batch holds (rid_min > rid_max: none)
    uint32_t n_pending;     // candidates set aside, all read groups together (a shard_tail context): the length of the batch's pending log
    uint32_t first_certain; // one read group: candidate index of the first read that resets whatever the state (0xFFFFFFFF: none; only
                            // looked for while setting aside).  Several: every group has its own (AnchorArgs::lane_fc)
    uint32_t n_bad;         // reads whose lane is >= n_lanes (they end the run on the card: k_prep's check 2); counted with several read groups only
    uint32_t pad;
    unsigned long long seq_bytes, qual_bytes, cigar_words; // payload sizes: sums of ceil(l_seq / 2), l_seq, n_cigar
};
// one read group's part (k_an_chain): its window state, its reads, where its candidates and its first_of segment lie.  One read group:
// lanes[0] with cand_off = first_off = 0 and n_reads = n (a lane out of range is not looked for: n_bad = 0)
struct AnchorLane {
    AnchorState before, after;
    uint32_t n_cand, n_reads; // candidates / all reads of the read group in the batch
    uint32_t cand_off;        // its first candidate in the compaction (the candidates grouped by read group, stream order inside a group)
    uint32_t first_off;       // its segment of first_of: last_rel + 1 entries (none when it has no anchored candidate), the groups' back to back
    uint32_t last_rel;        // window (relative to before.win) of its last candidate
    // a shard_tail context whose read group is still setting aside (before.pending): the group's first n_pending candidates are set
    // aside — those in front of ITS first certain reset —, and their entries of the batch's pending log are pend_base .. pend_base +
    // n_pending - 1, in stream order (the groups' parts back to back in group order; resolve steps one state per group, so any log
    // that keeps a group's reads in stream order is the stream's)
    uint32_t n_pending, pend_base;
    uint32_t pad;
};
#define AN_FLAG_TOO_MANY_BREAKS 1u // not anchored: the state is untouched, the caller takes the host's recurrence for this batch
#define AN_FLAG_BOUND_OVERFLOW  2u // never expected (the list is sized for every candidate)

#define AN_NO_READ 0xFFFFFFFFu // first_of[rel]: no candidate's window changes TO rel (a reset skips one)

// a run = a break and the candidates behind it up to the next break: inside it every gap is in [0, 1000) on one chromosome, so a
// read's state follows in closed form from the state the run was entered with
struct AnchorRun {
    uint32_t b_e;     // beginPos of the run's first read
    uint32_t s_e;     // shift after that read
    uint32_t rel_e;   // window (relative to before.win) after that read
    uint32_t stuck;   // that read sits at offset 2000 exactly (neither slide nor reset): reads at the same position stay there, the first
                      // one further right resets
    uint32_t b_star;  // stuck: beginPos of that first read further right (if the run has one)
};

// breaks a batch may hold for the card's chain (ONE thread walks them, ~0.2 us each: 3 ms at this limit, what the host's pass over a
// million reads takes); a batch with more — sparse data: every other read is a break — is left to the host.  With several read groups
// the limit is over the whole batch, not per group: the breaks of all groups share bj[] / runs[], and the groups' walks run side by
// side, so that no walk is longer than the one-group walk at this limit
#define AN_MAX_BREAKS 16384u

struct AnchorPart { // what a workgroup of k_an_count (1024 reads) knows; summed by k_an_scan
    uint32_t n_slow, max_slow, n_noqual, first_certain;
    int32_t rid_min, rid_max;
    unsigned long long s1, s2, s3;
};

struct AnchorArgs {
    uint32_t n, n_refs, n_lanes, no_fast;
    uint32_t lane_bits;         // several read groups: ballots that tell the read groups apart (ceil(log2(n_lanes)))
    uint32_t set_aside;         // several read groups: a shard_tail context that is not resolved — some state[] may be pending
    const uint16_t* flag; const uint8_t* lane; const int32_t* rid; const int32_t* pos; const uint32_t* l_seq; const uint16_t* n_cigar;
    const uint8_t* main_chrom;
    CovEntry* cov_out;          // [n]
    AnchorState* state;         // [n_lanes] the read groups' states: read by the chain, replaced when the batch is anchored
    AnchorSummary* sum;
    AnchorLane* lanes;          // [n_lanes]
    // first_of[rel] = the first read (index in the batch) whose window is `rel`, written by the candidate whose window differs from its
    // predecessor's (windows only grow along the candidates, by one per slide and two per reset: rel <= 2 n_cand + 2); preset to AN_NO_READ.
    // (Round 4, first version: a list appended to with an atomic counter — ~5 000 returning atomics on ONE word per million reads,
    // 60 of k_an_apply's 83 us.)
    // Several read groups: one such table per read group present, at lanes[l].first_off; indices stay stream-order read indices.
    uint32_t* first_of; uint32_t first_cap;
    // scratch
    uint32_t* cpos; int32_t* crid; uint32_t* cidx; uint32_t* crun; // [n] candidates in stream order (several read groups: grouped by read group)
    uint8_t* clane;             // [n] several read groups: the candidate's read group
    uint32_t* bj;               // [AN_MAX_BREAKS] candidate index of every break
    AnchorRun* runs;            // [AN_MAX_BREAKS]
    uint32_t* blk_a; uint32_t* blk_b; // [n / 1024 + 2] block counts / offsets of the two compactions
    AnchorPart* parts;          // [n / 1024 + 2]
    uint32_t* blk_c;            // several read groups: [n_lanes][n / 1024 + 2] candidates per read group and workgroup (scanned in place)
    uint32_t* blk_r;            // ... [n_lanes + 1][n / 1024 + 2] reads per workgroup and bin (bin 0: lane >= n_lanes, bin l + 1: read group l)
    // several read groups, set_aside: every group's first certain reset (candidate index; 0xFFFFFFFF: none), and the batch's pending log
    // (chromosome, beginPos and read group of the reads set aside, by their index in the log)
    uint32_t* lane_fc;          // [n_lanes]
    int32_t* plog_rid; uint32_t* plog_bp; uint8_t* plog_lane; // [n]
};

extern "C" void bqc_launch_anchor(const AnchorArgs& a, hipStream_t s);
// the processing order of a batch with several read groups, on the card: reads with a lane >= n_lanes first, then read group 0, 1, ...,
// stream order inside each (bqc_pipeline.cpp: host_pass builds the same permutation on the host); tmp: lane_order_tmp_words() words
extern "C" void bqc_launch_lane_order(const uint8_t* lane, uint32_t n, uint32_t n_lanes, uint32_t* order, uint32_t* tmp, hipStream_t s);
static inline size_t lane_order_tmp_words(uint32_t n, uint32_t n_lanes) { return ((size_t)n + 1023) / 1024 * ((size_t)n_lanes + 1) + 64; }
