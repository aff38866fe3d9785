// bqc_ctx.h — the context behind include/bamqc.h, shared by bqc_api.cpp (life cycle, state vector, finalisation) and
// bqc_pipeline.cpp (host pass, staging ring, uploads and launches).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bamqc.h"
#include "device_types.h"
#include "prep.h"
#include "anchor.h"
#include "sketch.h"
#include "../host/raw_vector.h"

struct LaneCov { // host side of OverallNumbers' window state machine (OverallNumbers.hpp:84-110)
    bool first = true;
    int32_t id = 0;
    uint32_t shift = 0;      // (unsigned as the reference's arithmetic: anchor.h, an_step)
    uint64_t win = 0;        // absolute index (flush order) of the window currently held in v1
    uint64_t batch_base = 0; // absolute window index that is batch-relative window 0 (= carry windows 0,1)
};

// What the host knows about a batch after its pass over the fixed columns (bqc_pipeline.cpp: host_pass).
struct HostPass {
    uint32_t n = 0;
    uint64_t seq_bytes = 0, qual_bytes = 0, cigar_words = 0;
    uint32_t n_slow = 0, max_len_slow = 0;  // reads for the generic kernels, the longest of them
    uint32_t t8_lane = 0;                   // read group with the most reads (k_long: its per-cycle tiles go through the scratch array)
    bool multi_lane = false;
    raw_vector<CovEntry> cov;               // [n] anchors {win, pos} / BQC_COV_NONE
    raw_vector<uint32_t> order;             // [n] reads grouped by read group (only when multi_lane)
    std::vector<SuperWindow> sws;
    std::vector<Stretch> stretches;
    std::vector<CovTile> tiles;
    std::vector<uint8_t> lane_mask, started_after;
    std::vector<uint64_t> add_idx, add_val; // host-computed additions (zero-depth windows)
    uint32_t n_pending = 0;                 // shard mode: reads marked BQC_COV_PENDING in `cov` (their log: ShardCtx::batches.back())
    // scratch kept from batch to batch
    std::vector<std::vector<uint32_t>> lane_first; // per read group: first read index whose window is >= k
    std::vector<uint64_t> lane_count;
};

// A batch in device memory: one allocation, carved into the uploaded columns, the host pass's tables and the outputs of the
// device pre-pass.
struct BatchMem {
    void* dmem = nullptr;
    size_t dcap = 0;
    DevBatch d{};
    PrepArgs prep{};
    uint8_t* d_lane_mask = nullptr;
    uint8_t* d_started_after = nullptr;
    uint64_t* d_add_idx = nullptr;
    uint64_t* d_add_val = nullptr;
    uint32_t n_add = 0;
    uint32_t* d_rsum = nullptr;          // [n_reads][3] per-read sums of the long-read kernel
    uint32_t* d_order_tmp = nullptr;     // an anchored batch with several read groups: scratch of bqc_launch_lane_order (its order is made on the card)
    ErrRec* d_err = nullptr;
    uint64_t algo_bytes = 0;
    uint32_t n_slow = 0, max_len_slow = 0, n_chunks_slow_ub = 0, t8_lane = 0;
    uint64_t lane_bits[4] = {0, 0, 0, 0}; // read groups the batch holds (their 8-mer counts may be in the scratch rows after its kernels)
    bool processed = false;
    // where the pieces of the host-side image go (offsets into dmem; the staged image has the same layout from h2d_begin on)
    size_t h2d_begin = 0, h2d_end = 0;   // the contiguous part that is copied from the staging image
    size_t o_col[13] = {0};              // flag mapq lane rid pos tlen nm as l_seq n_cigar seq qual cigar
    size_t col_bytes[13] = {0};
    size_t o_xr = 0, o_xv = 0, o_cov_in = 0, o_order = 0, o_sws = 0, o_stretch = 0, o_tiles = 0, o_mask = 0, o_started = 0, o_aidx = 0, o_aval = 0;
};

// Shard mode (bqc_options.shard_tail): the coverage reads set aside until the predecessor shard's final state is known.
struct PendBatch {                 // those of one batch, in stream order
    std::vector<uint8_t> lane;
    std::vector<int32_t> rid;
    std::vector<uint32_t> bp;
    void* dmem = nullptr;          // device: PendRun[n] | counter | PendExtra[extra_cap]
    uint32_t extra_cap = 0;
    uint32_t n() const { return (uint32_t)lane.size(); }
};
struct ShardCtx {
    bool tail = false, resolved = false, exported = false;
    std::vector<uint8_t> pending;  // [lane] 1: the read group's reads are still being set aside
    std::vector<uint8_t> has_prev; // [lane] the read before (of those that enter coverage): for the test "resets whatever the state"
    std::vector<int32_t> prev_rid;
    std::vector<uint32_t> prev_bp;
    std::deque<PendBatch> batches;
};

struct bqc_dbatch {
    BatchMem m;
    // host stream state after this batch (restored by bqc_process after a bqc_reset, see there)
    std::vector<LaneCov> cov_after;
    uint64_t seq = 0;
};

struct Slot { // one batch in flight through bqc_submit / bqc_submit_async
    BatchMem m;
    char* hmem = nullptr;     // page-locked staging image (host pass tables; the columns too on the staging path)
    size_t hcap = 0;
    ErrRec* h_err = nullptr;  // page-locked copy of the batch's error record (written by a D2H copy behind its last kernel)
    hipEvent_t ev_h2d = nullptr, ev_done = nullptr;
    bool busy = false;
    bool in_place = false;    // the batch's columns are read where the caller has them (bqc_submit_anchored): bqc_batch_uploaded waits for ev_done
    uint64_t ticket = 0;
};

// Anchors made on the card (anchor.h, k_anchor.hip) for batches whose columns live in device memory: bqc_anchor_enqueue /
// bqc_anchor_complete run in the thread that decodes the batches, bqc_submit_anchored in the one that submits them.
struct bqc_anchored {
    AnchorSummary* h_sum = nullptr;   // page-locked: the batch's summary ...
    AnchorLane* h_lanes = nullptr;    // ... its per-group part behind it (n_lanes entries) ...
    uint32_t* h_bound = nullptr;      // ... and the first kInline entries of first_of[] (anchor.h)
    std::vector<uint32_t> rest;       // the entries behind them (sparse data), fetched by bqc_anchor_complete
    std::vector<int32_t> pend_rid;    // a shard_tail context: the reads set aside (the batch's pending log, AnchorLane::pend_base) ...
    std::vector<uint32_t> pend_bp;    // ... chromosome and beginPos, for the pending log (bqc_shard_resolve) ...
    std::vector<uint8_t> pend_lane;   // ... and with several read groups the read group
    const CovEntry* d_cov = nullptr;  // the caller's device buffer with the anchors of the batch's reads
    uint32_t n = 0;
    bool completed = false;
    bool released = false;            // on the engine's free list
    static const uint32_t kInline = 1u << 17;
};
struct AnchorEngine {
    std::atomic<int> mode{0};         // 0: not used yet, 1: the card keeps the state, 2: off for the rest of the stream (the host keeps it)
    AnchorState* d_state = nullptr;   // [n_lanes] one window state per read group
    AnchorSummary* d_sum = nullptr;   // the summary, and AnchorLane[n_lanes] behind it
    uint32_t* d_bound = nullptr;
    void* d_scratch = nullptr;
    const uint32_t* d_plog_bp = nullptr; const int32_t* d_plog_rid = nullptr; const uint8_t* d_plog_lane = nullptr; // the outstanding batch's pending log (in the scratch)
    size_t cap_n = 0;                 // reads the scratch buffers are sized for
    std::mutex m;                     // the free list and `outstanding` (handles come back from the submitting thread)
    std::vector<bqc_anchored*> free_list, all;
    bqc_anchored* outstanding = nullptr; // enqueued, not yet completed or discarded: its summary and window table are in the scratch
                                         // buffers, which are single: bqc_anchor_enqueue refuses another batch until then
    std::string err;
};

// The optional modules' segments of the flat state vector, in the vector's order: [sl.words][sketch], then these.  The order is ABI
// (vectors are exchanged between processes) and is stated here and nowhere else: bqc_state_words, the four exchange calls, bqc_reset
// and bqc_destroy walk bqc_ctx::seg, and a segment's offset is the sum of the words in front of it (bqc_api.cpp: seg_start).
enum Seg {
    SEG_WDP,  // depth in fixed genome windows: [n_lanes][4 + 3 NW]
    SEG_RCV,  // depth over given regions: [n_lanes][4 + B + R]
    SEG_SAC,  // allele counts at given sites: [n_lanes][S][8: strand x base]
    SEG_SBC,  // substitutions: [n_lanes][2 mates]{X [2 strands][64][4], Y [N][16]}
    SEG_IBC,  // indels: [n_lanes][2 mates]{[3: E, IC, DC][N], [2: IL, DL][64]}
    SEG_GCB,  // GC bias: [n_lanes][3: R, B, Q][101]
    SEG_ADP,  // adapter content by cycle: [n_lanes][2][9: slots 0..7, then E][N]
    SEG_MBC,  // mismatches by cycle and base quality: [n_lanes][2][2: A, M][N][224]
    SEG_QCYC, // base quality by cycle: [n_lanes][2][N][224]
    N_SEG,
    MOD_DUP = N_SEG, // the duplicate sets: a module with views (bqc_ctx::finalised), no part of the vector
    MOD_OVR,         // the overrepresented sequences: the same
    N_MOD
};
struct StateSeg {
    uint64_t* d = nullptr; // the module's words in device memory (nullptr: the module is off)
    uint64_t words = 0;
};

struct bqc_ctx {
    bqc_options opt{};
    std::vector<uint8_t> main_chrom;
    std::vector<int32_t> fasta_index;
    StateLayout sl{};
    int device = 0;
    hipStream_t stream = nullptr;      // compute: every kernel of the context, in batch order
    hipStream_t copy_stream = nullptr; // host-to-device copies of the batches in flight
    // coverage beside the chunk plan (bqc_pipeline.cpp, enqueue_kernels): k_cov and its companions of a batch run on a stream of lower
    // priority between two events of the compute stream — forked behind k_prep_reads, joined before the batch's last launch
    hipStream_t cov_stream = nullptr;  // (made when the first batch needs it)
    bool cov_side = true;              // BQC_COV_STREAM=0: the coverage launches on the compute stream, behind k_long (as before round 8)
    hipEvent_t ev_cov_fork = nullptr, ev_cov_join = nullptr;
    uint32_t n_cu = 256;
    uint64_t* d_state = nullptr;
    ErrRec* d_err0 = nullptr;          // error record of work outside a batch (final flush)
    int32_t* d_cursor = nullptr;       // FASTA cursor of the stream (TripletCounting.hpp:254-259), device resident
    int32_t* d_fasta_index = nullptr;
    // 8-mer scratch rows of k_short: every workgroup of a launch owns a slot of BQC_T8_SPW rows (64 KiB images of its packed LDS
    // counters, written with plain stores); d_t8used[slot] = rows written.  The slots of up to kT8Launches launches pile up
    // and are summed into d_state by fold_t8: before the state is read, when the table is full, or when another read group
    // needs it.  (kT8Slots * BQC_T8_SPW * 64 KiB = 512 MiB of the 288 GB.)
    uint32_t* d_t8rows = nullptr;
    uint32_t* d_t8used = nullptr;
    // per-cycle counter tiles of k_long's workgroups (48 KiB each; d_kl_cyc_used[wg] = written), summed by k_long_cyc_fold in the same launch
    uint32_t* d_kl_cyc = nullptr;
    uint32_t* d_kl_cyc_used = nullptr;
    uint32_t kl_slots_cap = 0;  // workgroups d_kl_cyc / d_kl_cyc_used have room for (bqc_long_slots_cap)
    uint32_t t8_slots_used = 0, t8_slots_cap = 0;
    uint64_t t8_lanes[4] = {0, 0, 0, 0}; // read groups (bit per lane) of the batches whose rows are in the table
    std::vector<std::pair<void*, size_t>> pool; // device buffers of freed batches, reused by bqc_upload (hipMalloc / hipFree cost milliseconds)
    uint32_t* d_carry = nullptr;  // [lane][2][2000]
    uint32_t* d_parity = nullptr; // [lane], then the count of finished workgroups of the running k_cov
    uint8_t* d_started = nullptr; // [lane]
    // references
    std::vector<uint8_t*> d_ref;
    // bqc_reserve_references: one allocation the contigs are carved from (an allocation behind a running kernel waits for it: a
    // caller that uploads contigs while batches run reserves first); pointers inside it are not released one by one
    uint8_t* ref_arena = nullptr;
    size_t ref_arena_cap = 0, ref_arena_used = 0;
    std::vector<uint32_t*> d_refn; // one-hot nibble copy for the short-read fast path
    std::vector<uint64_t> ref_len;
    uint8_t** d_ref_ptrs = nullptr;
    uint32_t** d_refn_ptrs = nullptr;
    bool no_fast = false;          // BQC_NO_FAST=1: every read takes the generic kernel
    uint64_t* d_ref_len = nullptr;
    uint8_t* d_main = nullptr;
    // coverage host state
    std::vector<LaneCov> cov;
    bool flushed = false;
    bool poisoned = false;
    int poison_code = 0;
    uint64_t upload_counter = 0; // number of batches passed so far
    uint64_t state_seq = 0;      // sequence number of the batch the host stream state (cov) reflects
    HostPass hp;                 // host pass of the batch being submitted (its vectors are reused)
    ShardCtx shard;
    // batches in flight
    static const int kSlots = 3;
    Slot slots[kSlots];
    uint64_t next_ticket = 1;    // ticket of the next submitted batch; slot = ticket % kSlots
    uint64_t checked_ticket = 0; // every batch up to here has been waited for and its error record read
    AnchorEngine anchor;
    // sketch (N1)
    SketchDevice* sketch = nullptr;
    // the optional modules (each: nothing of it exists while it is off)
    StateSeg seg[N_SEG];               // their words of the state vector
    bool finalised[N_MOD] = {};        // per module: bqc_finalize has made its views since the last bqc_reset
    bool modules_closed = false;       // state has been exported, imported or finalised: the bqc_enable_* calls come too late
    // per-cycle base quality histograms (k_qcyc.hip; bqc_options.qual_by_cycle = N, 0: off — nothing below exists then)
    std::vector<uint64_t> h_qcyc;      // bqc_finalize's copy, and per (lane, mate) the printed sizes
    std::vector<uint32_t> qcyc_ncyc, qcyc_nq;
    // mismatches by cycle and base quality (k_mbc.hip; bqc_options.mismatch_by_cycle = N, 0: off — nothing below exists then)
    std::vector<uint64_t> h_mbc;       // bqc_finalize's copy, and per (lane, mate) the printed sizes
    std::vector<uint32_t> mbc_ncyc, mbc_nq;
    // adapter content by cycle (k_adp.hip; bqc_modules.adapter_by_cycle = N through bqc_create_ex, 0: off — nothing below exists then)
    uint32_t adp_n = 0;                // the capacity N
    std::vector<std::string> adp_names, adp_seqs; // the set in use: the context's own copies
    std::vector<bqc_adapter> adp_set;  // ... as bqc_adp_view shows it
    AdpPatterns adp_pat{};
    std::vector<uint64_t> h_adp;       // bqc_finalize's copy, and per (lane, mate) the printed length
    std::vector<uint32_t> adp_ncyc;
    // GC bias (k_gcb.hip; bqc_enable_gc_bias(W) after creation — nothing below exists without it)
    uint32_t gcb_w = 0;                // the window length W
    GcbDiv gcb_div{};                  // the reciprocals of W - n, n = 0..4
    uint64_t* d_gcb_g = nullptr;       // [101] the genome table G: bqc_finalize's, not part of the state vector
    GcbContig* d_gcb_tab = nullptr;    // [n_refs] the contigs of the genome table's launch
    std::vector<uint64_t> h_gcb, h_gcb_g; // bqc_finalize's copies
    // indels by cycle and by length (k_ibc.hip; bqc_enable_indel_by_cycle(N) after creation — nothing below exists without it)
    uint32_t ibc_n = 0;                // the cycle capacity N
    std::vector<uint64_t> h_ibc;       // bqc_finalize's copy, and per (lane, mate) the printed length
    std::vector<uint32_t> ibc_ncyc;
    // substitutions by context and by cycle (k_sbc.hip; bqc_enable_substitutions(N, Q, MQ) after creation — nothing below exists without it)
    uint32_t sbc_n = 0, sbc_q = 0, sbc_mq = 0; // the cycle capacity N, the minimum base quality, the minimum mapping quality
    std::vector<uint64_t> h_sbc;       // bqc_finalize's copy, and per (lane, mate) the printed length
    std::vector<uint32_t> sbc_ncyc;
    // allele counts at given sites (k_sac.hip; bqc_enable_site_alleles(sites, Q, MQ) after creation — nothing below exists without it)
    uint32_t sac_s = 0, sac_q = 0, sac_mq = 0; // the number of sites S, the minimum base quality, the minimum mapping quality
    void* d_sac_tab = nullptr;         // the site tables of `sac_sites`, one allocation
    SacSites sac_sites{};
    std::vector<int32_t> sac_rid, sac_pos; // the list as given (bqc_site_alleles' view)
    std::vector<uint64_t> h_sac;       // bqc_finalize's copy
    // depth in fixed genome windows (k_wdp.hip; bqc_enable_window_depth(W, lengths, MQ) after creation — nothing below exists without it)
    void* d_wdp_tab = nullptr;         // the tables of `wdp_tab`, one allocation
    WdpTab wdp_tab{};
    uint32_t wdp_mq = 0;               // the minimum mapping quality of the class `good`
    std::vector<uint32_t> wdp_len, wdp_woff; // the contigs' lengths and first windows (n_refs + 1) as the view shows them
    std::vector<uint64_t> h_wdp, h_wdp_contigs, h_wdp_hist; // bqc_finalize's copy of the words, [n_lanes][n_refs][3] and [n_lanes][1001]
    // depth over given regions (k_rcv.hip; bqc_enable_region_coverage(regions, MQ, thresholds, D) after creation — nothing below exists without it)
    uint32_t rcv_r = 0, rcv_mq = 0;    // the number of regions R, the minimum mapping quality
    uint64_t rcv_b = 0;                // B: the regions' bases
    void* d_rcv_tab = nullptr;         // the region tables of `rcv_regions`, one allocation
    RcvRegions rcv_regions{};
    RcvFinal rcv_fp{};                 // the finalize parameters: thresholds and the histogram's cap (not part of the state)
    uint64_t* d_rcv_out = nullptr;     // k_rcv_final's products and, behind them, its tile sums
    uint64_t rcv_out_words = 0;
    std::vector<int32_t> rcv_rid, rcv_start, rcv_end; // the list as given (bqc_region_coverage's view)
    std::vector<uint64_t> rcv_thr;     // the thresholds as the view shows them
    std::vector<uint64_t> h_rcv_out, h_rcv_eta; // bqc_finalize's copies: the products, and [n_lanes][4: E, T, A, bases on target]
    // duplicate sets by alignment signature (k_dup.hip; bqc_enable_duplicate_sets(capacity) after creation — nothing below exists without it,
    // and none of it is part of the state vector)
    DupTable dup_tab{};                // the table's slots (d_dup), the counter of sets behind them, C - 1 and the capacity
    void* d_dup = nullptr;             // one allocation: [C slots][n_sets, 7 spare words][n_lanes][5 sums][k_dup_final's products]
    uint64_t* d_dup_sums = nullptr;    // [n_lanes][5: E_single, E_pair, F_single, F_pair, second ends]
    uint64_t* d_dup_out = nullptr;     // k_dup_final's products: [2][256] sets by size, the two largest sets
    std::vector<uint64_t> h_dup_out, h_dup_sums; // bqc_finalize's copies
    uint64_t dup_sets[2] = {0, 0}, dup_estimate = 0;
    // overrepresented sequences (k_ovr.hip; bqc_enable_overrepresented(K, ppm, capacity) after creation — nothing below exists without it,
    // and none of it is part of the state vector)
    DupTable ovr_tab{};                // the table's slots (d_ovr), the counter of sets behind them, C - 1 and the capacity
    void* d_ovr = nullptr;             // one allocation: [C slots][n_sets, 7 spare words][n_lanes][4 sums][k_ovr_final's products]
    uint64_t* d_ovr_sums = nullptr;    // [n_lanes][4: examined first, examined second, skipped first, skipped second]
    uint64_t* d_ovr_out = nullptr;     // k_ovr_final's products: BQC_OVR_HEAD words, then the list of ovr_list_cap sets
    uint32_t ovr_k = 0, ovr_ppm = 0;   // the prefix length K and the list's threshold in reads per million
    uint64_t ovr_list_cap = 0;         // 2 floor(10^6 / ppm): the sets both mates can list
    std::vector<uint64_t> h_ovr_out, h_ovr_sums; // bqc_finalize's copies
    uint64_t ovr_distinct[2] = {0, 0}, ovr_threshold[2] = {0, 0};
    std::vector<bqc_ovr_seq> ovr_listed; // the list as the view shows it: mate 0's sets, then mate 1's, each sorted
    std::vector<std::string> ovr_text;   // ... and its sequences' letters
    uint32_t ovr_n_listed[2] = {0, 0};
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev;
    std::vector<const char*> tnames;
    std::vector<float> tms;
    int n_timed = 0;
    // finalize output
    std::vector<uint64_t> h_state;
    std::vector<std::vector<uint64_t>> arrays;
    std::vector<bqc_lane_counts> lanes;
    std::vector<std::vector<bqc_sketch_counts>> sk_out;
    bqc_counts counts{};
    std::string err;
};

int bqc_fail(bqc_ctx* c, int code, const char* fmt, ...);
#define HIPCHK(c, call)                                                                                         \
    do {                                                                                                        \
        hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess) return bqc_fail(c, BQC_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// bqc_api.cpp: a non-blocking stream on `device` — one of those bqc_warmup has made ahead, or a new one (nullptr: creation failed);
// rank BQC_STREAM_RANK_COV: never made ahead, and of the lowest priority the device has
#define BQC_STREAM_RANK_COV 4
hipStream_t bqc_pool_stream(int device, int rank);
// the context's copy stream, taken when the first batch needs it (0: ok)
int bqc_copy_stream(bqc_ctx* c);
// bqc_pipeline.cpp
int bqc_report_errors(bqc_ctx* c, const ErrRec& e); // what the device found wrong with a batch -> error code + message (0: nothing)
int bqc_drain(bqc_ctx* c);                 // wait for every batch in flight; returns the first error of the stream (context poisoned)
void bqc_pipeline_destroy(bqc_ctx* c);     // frees slots and pooled buffers
hipError_t bqc_anchor_fresh_state(bqc_ctx* c); // every read group's window state on the card back to "no read yet" (d_state exists)
void bqc_anchor_destroy(bqc_ctx* c);       // frees the anchor engine's buffers and handles
// Every reader of d_state goes through this: the packed 8-mer rows of k_short are summed into the state vector first.
void bqc_state_ready(bqc_ctx* c);
