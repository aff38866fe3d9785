// prep.h — arguments of the device-side pre-pass (k_prep.hip), filled by the host pipeline (bqc_pipeline.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_types.h"

// Payload offsets come from two levels of sums: k_prep_sizes has one workgroup per group of PR_GROUP consecutive blocks of 1024 reads
// and leaves, per block, the sums of the blocks before it inside its group, and per group its totals; k_prep_reads adds the totals
// of the groups before its own.  A power of two, at least 16 (a wave of k_prep_sizes per block, 16 waves).
#ifndef PR_GROUP
#define PR_GROUP 32
#endif
static_assert(PR_GROUP >= 16 && (PR_GROUP & (PR_GROUP - 1)) == 0, "PR_GROUP: a power of two, 16 or more");

// Bases of a block's three payload quantities (ceil(L/2), L, n_cigar) from the totals of the groups before its group (`before`) and
// the sums inside its group up to the block, without it (`excl`) and with it (`incl`).  True: the block's inclusive end exceeds
// 32-bit offsets in some quantity — the batch is refused at the first such block (key: its first read << 3 | 3).
__host__ __device__ inline bool prep_block_bases(const unsigned long long before[3], const unsigned long long excl[3], const unsigned long long incl[3],
                                                 unsigned long long base[3])
{
    bool over = false;
    for (int k = 0; k < 3; ++k) {
        base[k] = before[k] + excl[k];
        over |= before[k] + incl[k] > 0xFFFFFFFFull;
    }
    return over;
}

struct Stretch {          // the reads of one read group, contiguous in processing order: super-windows [sw_begin, sw_end)
    uint32_t lane, sw_begin, sw_end, pad;
};

struct PrepArgs {
    uint32_t n;               // reads
    uint32_t n_lanes, max_read_len;
    uint32_t no_fast;         // BQC_NO_FAST=1: every read takes the generic kernels
    uint32_t replay;          // the batch has been processed before (bqc_process on a resident batch): start from its saved FASTA cursor
    // raw columns (as uploaded)
    const uint16_t* flag_in;
    const uint8_t* mapq;
    const uint8_t* lane;
    const int32_t* rid;
    const int32_t* pos;
    const int32_t* as_;
    const uint32_t* l_seq;
    const uint16_t* n_cigar;
    const uint8_t* qual;
    const uint32_t* cigar;
    const CovEntry* cov_in;   // host anchor pass: {win, pos} or BQC_COV_NONE
    const uint32_t* order;    // processing order (reads grouped by read group) or nullptr
    const SuperWindow* sws;
    uint32_t n_sw;
    const Stretch* stretches;
    uint32_t n_stretch;
    const int32_t* fasta_index; // [n_refs] position of the contig in FASTA order (-1: absent) or nullptr = identity
    // outputs
    uint16_t* flag_out;
    uint32_t* seq_off;
    uint32_t* qual_off;
    uint32_t* cigar_off;
    CovEntry* cov_out;
    CovExtra* cov_extra;
    uint32_t cov_extra_cap;
    PendRun* pend;            // shard mode: covered runs of the reads marked BQC_COV_PENDING (retained until bqc_shard_resolve)
    PendExtra* pend_extra;
    uint32_t* pend_extra_n;
    uint32_t pend_extra_cap;
    uint16_t* cls;            // per read: class << 8 | triplet segments (class 0 / 1: fast read by mate slot, 2: generic path)
    TripSeg* segs;            // at cigar_off[r] + j
    uint32_t* perm;
    uint32_t perm_cap;
    Chunk* chunks_fast;
    uint32_t chunks_fast_cap;
    Chunk* chunks_slow;
    uint32_t chunks_slow_cap;
    BatchDesc* desc;
    ErrRec* err;
    int32_t* cursor;          // FASTA cursor of the stream (TripletCounting.hpp:254-259), device resident
    int32_t* cursor_save;     // its value before this batch
    // scratch
    unsigned long long* blk_sizes; // [blocks][3] sums of the blocks before this one inside its group of PR_GROUP blocks
    unsigned long long* grp_sizes; // [groups][3] totals of every group
    uint32_t* blk_tgt;        // [blocks][2] max / min FASTA position + 1 of the block's eligible reads
    uint32_t* blk_maxfast;    // [blocks][2] longest fast read, longest generic read
    SwCounts* sw_counts;
    SwPlan* sw_plan;
};

extern "C" void bqc_launch_prep(const PrepArgs& a, const DevRefs& refs, hipStream_t s, hipEvent_t after_reads);
// host: what the two kernels compute from block totals [n_blocks][3] — bases [n_blocks][3]; returns the first block whose inclusive end
// exceeds 32-bit offsets, 0xFFFFFFFF: none (tests: a batch that large cannot be a test)
extern "C" uint32_t bqc_prep_bases(const uint64_t* blk_totals, uint32_t n_blocks, uint64_t* bases);
extern "C" uint32_t bqc_prep_group(void);
// shard mode: intervals of a batch's pending reads once the host knows their windows (cov_in = {win, pos} per pending read)
extern "C" void bqc_launch_pend_cov(uint32_t n, const CovEntry* cov_in, const PendRun* pend, const PendExtra* extra, const uint32_t* extra_n, uint32_t extra_cap,
                                    const uint8_t* lane, CovEntry* cov_out, CovExtra* cov_extra, BatchDesc* desc, hipStream_t s);
