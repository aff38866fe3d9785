/*
 * bamqc.h — C ABI of the MI355X-native per-read aggregation path of BamQC.
 *
 * The reference (DecodeGenetics/BamQC) has no FFI: its hot path is the body of
 * the `while (!atEnd(inStream))` loop in src/bamqualcheck.cpp:303-444, which
 * calls member functions on `struct Counts` (src/bamqualcheck.cpp:14-38).
 * This header is the seam "loop body <-> Counts": a host that has decoded BAM
 * records hands them over as structure-of-arrays batches, the library
 * aggregates them on the GPU, and `bqc_finalize` returns a host mirror of
 * `Counts` that a writer turns into the `.bamqc` text
 * (src/bamqualcheck.cpp:156-233).
 *
 * Plain C, no exceptions cross the boundary, every entry point returns
 * 0 = ok / non-zero = error with a message retrievable via bqc_last_error()
 * (mirrors the reference's "message on stderr + return 1",
 * src/bamqualcheck.cpp:265,281,308,315,341,388).
 *
 * Threading: one submitting thread per context (the reference is
 * single-threaded).
 */
#ifndef BAMQC_H_
#define BAMQC_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BQC_ABI_VERSION 2

/* ---- error codes ---------------------------------------------------------- */
enum {
    BQC_OK = 0,
    BQC_ERR_ARG = 1,          /* bad argument / inconsistent batch                              */
    BQC_ERR_DEVICE = 2,       /* HIP runtime error (no GPU, OOM, launch failure)                */
    BQC_ERR_NO_MATE_FLAG = 3, /* neither 0x40 nor 0x80 set   (bamqualcheck.cpp:385-389)         */
    BQC_ERR_AS_TAG = 4,       /* AS tag missing/negative on a read that passed flags+mapQ
                                 (TripletCounting.hpp:116-127,154-155 -> bamqualcheck.cpp:340)  */
    BQC_ERR_FASTA = 5,        /* contig needed for triplets is missing from / behind the FASTA
                                 cursor (TripletCounting.hpp:85-104,254-259)                    */
    BQC_ERR_RANGE = 6,        /* value exceeds a configured capacity (read length, histogram)   */
    BQC_ERR_IO = 7,           /* file could not be opened / parsed                              */
    BQC_ERR_STATE = 8         /* call sequence error                                            */
};

/* ---- scalar counters of OverallNumbers (OverallNumbers.hpp:12-24) ---------- */
enum {
    BQC_S_SUPPLEMENTARY = 0,
    BQC_S_DUPLICATES,
    BQC_S_QCFAILED,
    BQC_S_NOT_PRIMARY,
    BQC_S_READCOUNT,
    BQC_S_TOTALBPS,
    BQC_S_BOTHUNMAPPED,
    BQC_S_FIRSTUNMAPPED,
    BQC_S_SECONDUNMAPPED,
    BQC_S_FIRST_AND_OR_SECOND_MAPPED,
    BQC_S_FF_RR,
    BQC_S_PROPERPAIR,
    BQC_S_AUTO_PROPERPAIR,
    BQC_N_SCALARS
};

/* Host annotations carried in the spare high bits of the BAM flag column.     */
#define BQC_FLAG_MATE_MAIN 0x1000u /* rNextId is a main chromosome (bamqualcheck.cpp:404) */
#define BQC_FLAG_NO_QUAL   0x8000u /* the record has no qualities (BAM: quality block starts with 0xFF; SAM: QUAL is "*")
                                      => record.qual empty.  Set by whoever decodes the record: the library does not look
                                      at the quality bytes to find out (it would cost a cache line per read).             */

#define BQC_NM_ABSENT (-1)
#define BQC_AS_ABSENT INT32_MIN

#define BQC_COVSIZE 100   /* OverallNumbers.hpp:51 covsize */
#define BQC_VSIZE   1000  /* OverallNumbers.hpp:51 vsize   */
#define BQC_N_8MER  65536 /* OverallNumbers.hpp:53         */
#define BQC_N_TRIPLET (64 * 4 * 4)

/* ---- options -------------------------------------------------------------- */
typedef struct bqc_sketch_options { /* N1: ReadQualityHasher/StreamCounter (CommandLineParser.hpp:73-81) */
    uint32_t n_k;          /* number of k values (0 = sketch disabled)          */
    const int32_t* klist;  /* -k, default {32}; 1 <= k <= 63                     */
    uint32_t n_q;
    const uint32_t* qlist; /* -q, default {17}                                   */
    double e;              /* -e, default 0.01                                   */
    int32_t seed;          /* -s, default 1; 0 = table seeded from time(NULL), as RepHash.cpp:5-7 (not reproducible;
                              shards of one run must then be given the same non-zero seed by their driver)   */
} bqc_sketch_options;

typedef struct bqc_options {
    uint32_t struct_size;      /* sizeof(bqc_options), for ABI evolution                 */
    uint32_t n_lanes;          /* number of @RG IDs (bamqualcheck.cpp:296-298), >= 1     */
    uint32_t n_refs;           /* number of BAM reference sequences                      */
    int32_t isize;             /* -i (CommandLineParser.hpp:66-67), default 1000         */
    uint32_t max_read_len;     /* capacity of the per-cycle arrays (reference grows on
                                  demand, QualityCheck.hpp:85-105); longer read => BQC_ERR_RANGE */
    uint32_t hist_cap;         /* capacity of mismatch/deletion/insertion histograms     */
    const uint8_t* main_chrom; /* [n_refs] 1 = rID in chrIdset (bamqualcheck.cpp:106-123) */
    const int32_t* fasta_index;/* [n_refs] position of the contig in FASTA order, -1 =
                                  absent (TripletCounting.hpp:254-259); NULL = identity   */
    int32_t device;            /* HIP device ordinal                                     */
    bqc_sketch_options sketch;
    uint32_t shard_tail;       /* 1: this context processes a shard of the record stream that does NOT begin with the
                                  stream's first record (multi-GPU, see bqc_shard_resolve)              */
    uint32_t qual_by_cycle;    /* per-cycle base quality histograms (bqc_qual_by_cycle): 0 = off, else the cycle capacity N,
                                  1 <= N <= max_read_len; cycles at or behind N of a longer read are not counted.  (The field
                                  lies in what was the structure's tail padding: bqc_create takes the structure with or
                                  without it, and a caller that cleared the structure has the module off.)        */
    uint32_t mismatch_by_cycle;/* mismatches by cycle and base quality (bqc_mismatch_by_cycle): 0 = off, else the cycle capacity N,
                                  1 <= N <= max_read_len.  bqc_create also takes the structure as it was before this field
                                  (struct_size 8 smaller): the module is off then.                              */
    uint32_t pad_tail;         /* keeps sizeof a multiple of 8; not read                                         */
} bqc_options;

/* ---- input batch (host, structure of arrays) -------------------------------
 * Reads are stored back to back: read i owns
 *   seq   [ sum_{j<i} (l_seq[j]+1)/2 , +(l_seq[i]+1)/2 )   BAM-native 4-bit, high nibble first
 *   qual  [ sum_{j<i} l_seq[j]       , +l_seq[i] )          raw Phred bytes (no +33)
 *   cigar [ sum_{j<i} n_cigar[j]     , +n_cigar[i] )        BAM-native len<<4|op ("MIDNSHP=X")
 * All columns are in BAM orientation (as stored); the library applies the
 * reference's reverse-complement transform (bamqualcheck.cpp:345-350) itself.
 */
typedef struct bqc_batch {
    uint32_t n_reads;
    const uint16_t* flag;   /* BAM flag | BQC_FLAG_* host annotations                       */
    const uint8_t* mapq;
    const uint8_t* lane;    /* index from the RG:Z tag (bamqualcheck.cpp:72-100)            */
    const int32_t* rid;     /* refID, -1 = none                                             */
    const int32_t* pos;     /* 0-based leftmost position                                    */
    const int32_t* tlen;
    const int32_t* nm;      /* first integer-typed NM tag, BQC_NM_ABSENT if none            */
    const int32_t* as;      /* AS tag value, BQC_AS_ABSENT if none                          */
    const uint32_t* l_seq;
    const uint16_t* n_cigar;
    const uint8_t* seq;
    const uint8_t* qual;
    const uint32_t* cigar;
    /* further integer NM tags of a record (QualityCheck.hpp:201-218 loops over all of them) */
    uint32_t n_nm_extra;
    const uint32_t* nm_extra_read; /* read index, ascending */
    const int32_t* nm_extra_val;
} bqc_batch;

/* ---- output: host mirror of `struct Counts` -------------------------------
 * Every array is uint64_t; where the reference type is `unsigned`
 * (32-bit, OverallNumbers.hpp:12-24, QualityCheck.hpp:12-26) the value is
 * already reduced mod 2^32.  `n_*` are the reference's printed lengths
 * (arrays grow on demand there).
 */
typedef struct bqc_mate_counts {          /* QualityCheck (QualityCheck.hpp:8-56), r1 / r2        */
    uint32_t n_cycles;                    /* longest read seen = length of the per-cycle arrays   */
    const uint64_t* dnacount[5];          /* [n_cycles] A C G T N (Dna5 ordinal)                  */
    const uint64_t* qualcount;            /* [n_cycles] sum of (q-33) per cycle                   */
    uint64_t qualcount_readnr;            /* reads seen (unsigned)                                */
    const uint64_t* sc5;                  /* [n_cycles] scposcount_5prime                         */
    const uint64_t* sc3;                  /* [n_cycles] scposcount_3prime                         */
    uint32_t n_Ncount;      const uint64_t* Ncount;      /* n_cycles+1 (0 if no read)            */
    uint32_t n_GCcount;     const uint64_t* GCcount;
    uint32_t n_averageQual; const uint64_t* averageQual;
    uint32_t n_insertSize;  const uint64_t* insertSize;  /* isize+1, always                      */
    uint32_t n_mapQ;        const uint64_t* mapQ;
    uint32_t n_readLength;  const uint64_t* readLength;
    uint32_t n_mismatch;    const uint64_t* mismatch;
    uint32_t n_delhist;     const uint64_t* delhist;
    uint32_t n_inshist;     const uint64_t* inshist;
} bqc_mate_counts;

typedef struct bqc_sketch_counts {        /* one per (q,k): ReadQualityHasher (N1)                */
    uint32_t q, k;
    uint64_t sumCount, F0, f1, F2;
} bqc_sketch_counts;

typedef struct bqc_lane_counts {
    uint64_t scalars[BQC_N_SCALARS];
    uint64_t poscov[BQC_COVSIZE + 1];     /* genome_coverage_histogram                            */
    const uint64_t* eightmer;             /* [65536]                                              */
    bqc_mate_counts mate[2];
    const uint64_t* triplet;              /* [64 ctx][4: fwd1st, fwd2nd, rev1st, rev2nd][4 base]  */
    uint32_t n_sketch;                    /* n_q * n_k, q-major                                   */
    const bqc_sketch_counts* sketch;
} bqc_lane_counts;

typedef struct bqc_counts {
    uint32_t n_lanes;
    const bqc_lane_counts* lanes;
} bqc_counts;

typedef struct bqc_ctx bqc_ctx;
typedef struct bqc_dbatch bqc_dbatch; /* a batch resident in device memory */

/* ---- aggregation (replaces bamqualcheck.cpp:303-453) ----------------------- */
int bqc_abi_version(void);
int bqc_create(const bqc_options* opt, bqc_ctx** out);
/* Optional modules that are configured beside bqc_options, which stays as it is: bqc_create(opt, out) is bqc_create_ex(opt, NULL, out).
 * `mod` is checked with the other arguments, before the device is looked at; each of these is BQC_ERR_ARG with a message that names the
 * offending thing: a struct_size that is not sizeof(bqc_modules); adapter_by_cycle = 0 with adapters given; adapter_by_cycle >
 * max_read_len; more than 8 adapters; a sequence shorter than 8 or longer than 16; a letter outside ACGT; a bad or repeated name.
 * The context copies names and sequences: the caller's strings need not outlive the call.  (The adapter set: see bqc_adapter_by_cycle.) */
typedef struct bqc_adapter { const char* name; const char* seq; } bqc_adapter;
typedef struct bqc_modules {
    uint32_t struct_size;        /* sizeof(bqc_modules) of the caller */
    uint32_t adapter_by_cycle;   /* 0 = off, else the cycle capacity N, 1 <= N <= max_read_len */
    uint32_t n_adapters;         /* 0 = the built-in set */
    uint32_t pad;
    const bqc_adapter* adapters;
} bqc_modules;
int bqc_create_ex(const bqc_options* opt, const bqc_modules* mod, bqc_ctx** out);
/* Starts the HIP runtime on `device` (~0.06 s on a cold process) and makes the streams ahead that a context (and the program's reader)
 * will ask for (~0.05 s more, which then overlap with the caller's other set-up): callable from any thread, once per process, e.g.
 * while the inputs are opened. */
int bqc_warmup(int32_t device);
/* The FASTA order of the contigs (bqc_options.fasta_index) may also be given after creation, before the first batch: a
 * program can then create the context while it still reads the FASTA file. */
int bqc_set_fasta_index(bqc_ctx* ctx, const int32_t* fasta_index);
void bqc_destroy(bqc_ctx* ctx);
const char* bqc_last_error(const bqc_ctx* ctx); /* ctx may be NULL: last create error */

/* Reference chromosome as Dna5 codes (0..4 = A C G T N), one byte per base; the
 * library copies it to device memory (replaces Genome/readFastaRecord,
 * TripletCounting.hpp:60-104). */
int bqc_set_reference(bqc_ctx* ctx, int32_t rid, const uint8_t* dna5, uint64_t len);
/* Optional, before the first bqc_set_reference: one device allocation for contigs of total_bases bases in all, which
 * bqc_set_reference then carves from (an allocation made while kernels run waits for them). */
int bqc_reserve_references(bqc_ctx* ctx, uint64_t total_bases, uint32_t n_contigs);
/* The contigs of `from` become those of `to` without another upload (one process, many files: a context for another number of read
 * groups over the same genome).  Same device and n_refs; `to` has no reference yet.  `from` is only good for bqc_destroy afterwards. */
int bqc_move_references(bqc_ctx* from, bqc_ctx* to);
/* (ONE uploader thread may call bqc_set_reference while another thread submits batches — the program's non-default BQC_BG_REFS=1 mode —
 * under these rules: the contig is one no submitted batch has a read on; the uploader is the only caller of bqc_set_reference /
 * bqc_reserve_references at that time; and its error is read with bqc_last_error only after the submitting thread has stopped.  The call
 * waits for the context's compute stream: it returns when the batches queued before it are through.  No other concurrent use of a
 * context is supported, bqc_anchor_* beside bqc_submit_anchored excepted.) */

/* One batch of decoded records into the pipeline: host pass (coverage anchors), copy into a page-locked staging slot,
 * host-to-device copy, device pre-pass and kernels — three batches in flight, the call returns when the batch is queued.
 * The caller's buffers may be reused on return.  What the device finds wrong with a batch (the first failing read in
 * stream order, as the reference would have met it) surfaces at a later call: bqc_submit, bqc_sync, bqc_flush, bqc_finalize. */
int bqc_submit(bqc_ctx* ctx, const bqc_batch* batch);

/* The same without the staging copy, for callers whose columns live in page-locked memory (bqc_host_register, or
 * hipHostMalloc): the columns are copied to the device straight from the caller's memory and must stay untouched until
 * bqc_batch_uploaded(ctx, ticket, ...) returns 1.  The payload columns (seq, qual, cigar) may also live in the device's own
 * memory (a caller that inflates and decodes there); the fixed columns are read by the host as well and stay host pointers. */
int bqc_submit_async(bqc_ctx* ctx, const bqc_batch* batch, uint64_t* ticket);

/* ---- batches that live on the card entirely (a caller that decodes the records there: the program's reader, csrc/gpu_bam.hip) ----
 * With the FIXED columns in device memory too, the one order-dependent step of the reference's loop — the window state machine of
 * OverallNumbers::coverage, OverallNumbers.hpp:84-110, which bqc_submit* runs on the host over the fixed columns — runs on the card
 * as well (csrc/k_anchor.hip), and the columns never come to the host: it sees a summary of a few hundred bytes per batch.
 *   bqc_anchor_enqueue   queues the anchor kernels and the copy of their summary on `stream` (a hipStream_t on the context's device, on
 *                        which the columns are complete); d_cov: 8 bytes per read of device memory for the anchors, valid — like the
 *                        columns — until the batch's ticket is reported uploaded.  Returns 0 and a handle; 1: not available — a
 *                        batch has gone through bqc_submit* / bqc_upload before (the host then keeps the state for the rest of the
 *                        stream), or the context is a shard_tail context that bqc_shard_resolve has resolved; < 0: -BQC_ERR_*.  Any
 *                        number of read groups (n_lanes): one window state per read group on the card, and the batch's processing
 *                        order by read group is made there too.  A shard_tail context sets every read group's first reads aside on
 *                        the card — up to that group's own first certain reset — exactly as bqc_submit* does on the host.
 *   bqc_anchor_complete  after the caller has synchronised `stream`: 0 = anchored; 1 = not anchored (more position breaks in the batch —
 *                        all read groups together — than the card's chains take: the card has left every group's state untouched; this batch and every later one
 *                        go through bqc_submit* with host columns); < 0: -BQC_ERR_* (bqc_anchor_error).  `info` (optional): what a
 *                        program wants to know about a batch whose columns it does not have.
 *   bqc_submit_anchored  the batch into the pipeline as bqc_submit_async does (every column of `batch` a device pointer); consumes the handle.
 *                        The kernels read the columns IN PLACE (no copy into the pipeline's own buffers): they and d_cov must stay
 *                        untouched until bqc_batch_uploaded(ticket) says 1, which for such a batch means "its kernels are through";
 *                        at least 512 bytes of the same allocation must lie in front of and behind each of seq, qual and cigar (the
 *                        kernels' vector loads run over the ends).
 *   bqc_anchor_discard   returns a handle that bqc_submit_anchored will not consume (the caller's decode of the batch failed, or
 *                        bqc_anchor_complete said < 0).  The card's window state has already moved past that batch, so anchoring
 *                        ends with it: the next bqc_anchor_enqueue returns 1, and this batch and every later one go through
 *                        bqc_submit* with host columns.  After bqc_anchor_complete said 1 the handle is released already.
 * Batches must be anchored in stream order and submitted in the same order; the anchor calls may be made by another thread than the
 * submit calls (the program's decode thread and its submitting thread).  One handle at a time: while a handle is enqueued and
 * neither completed nor discarded, bqc_anchor_enqueue refuses the next batch with -BQC_ERR_STATE and leaves the card's state as it
 * is (the anchor kernels' scratch and summary buffers are single; completing k before enqueueing k+1 is what keeps k's window table).
 * Completed handles waiting for bqc_submit_anchored do not count: any number of those may be held. */
typedef struct bqc_anchored bqc_anchored;
typedef struct bqc_anchor_info {
    uint32_t n_noqual;        /* primary first / last records without qualities (check_read_len's message, QualityCheck.hpp:70-79) */
    int32_t rid_min, rid_max; /* range of the reference ids in [0, n_refs) the batch holds; rid_min > rid_max: none */
} bqc_anchor_info;
int bqc_anchor_enqueue(bqc_ctx* ctx, const bqc_batch* batch, void* d_cov, void* stream, bqc_anchored** out);
int bqc_anchor_complete(bqc_ctx* ctx, bqc_anchored* a, bqc_anchor_info* info);
int bqc_submit_anchored(bqc_ctx* ctx, const bqc_batch* batch, bqc_anchored* a, uint64_t* ticket);
void bqc_anchor_discard(bqc_ctx* ctx, bqc_anchored* a);
const char* bqc_anchor_error(const bqc_ctx* ctx);
/* 1: the batch's columns have been copied to the device (or the ticket is older than every batch in flight), 0: not yet
 * (only with wait == 0), < 0: -(BQC_ERR_*). */
int bqc_batch_uploaded(bqc_ctx* ctx, uint64_t ticket, int wait);
/* Page-lock / release host memory a caller decodes into (hipHostRegister; ~40 ms per GB once the pages are touched). */
int bqc_host_register(void* p, uint64_t bytes);
int bqc_host_unregister(void* p);

/* Same, split: keep the batch resident in HBM and run the hot path over it
 * any number of times (used by the benchmark, and by callers that overlap
 * upload with compute). */
int bqc_upload(bqc_ctx* ctx, const bqc_batch* batch, bqc_dbatch** out);
int bqc_process(bqc_ctx* ctx, bqc_dbatch* db);
void bqc_dbatch_free(bqc_ctx* ctx, bqc_dbatch* db);
uint64_t bqc_dbatch_bytes(const bqc_dbatch* db); /* algorithmic bytes resident for this batch */

int bqc_sync(bqc_ctx* ctx);  /* wait for all submitted work */
int bqc_reset(bqc_ctx* ctx); /* zero every counter (keeps references) */

/* End of stream: flush the two live coverage windows (bamqualcheck.cpp:447-453)
 * into the state vector.  Idempotent. */
int bqc_flush(bqc_ctx* ctx);

/* ---- shards of one record stream (multi-GPU) ------------------------------------------------------------------
 * Every statistic of the path is a sum over reads except the coverage-depth histogram: its window state machine
 * (OverallNumbers.hpp:84-110) depends on the reads before.  The stream may still be cut anywhere: a context created with
 * shard_tail = 1 sets aside, per read group, its reads up to the first one at which the state machine resets WHATEVER its
 * state (another chromosome, or more than 2000 positions away from the read before) and works normally from there on.
 * When all its batches are in: bqc_shard_resolve(predecessor's exported state) runs the reads set aside from the state the
 * predecessor ended in; bqc_shard_export yields this shard's own final state (its two live windows per read group are then
 * the successor's to flush: the state vector of a shard that has exported holds complete windows only).  The last shard
 * ends with bqc_flush / bqc_finalize as a whole stream does.  The exported block also carries the shard's first and last
 * FASTA position of triplet-eligible reads (words 0 and 1 of the block, int32, -1: none), so that the forward-only FASTA
 * scan (TripletCounting.hpp:254-259) can be checked across shards. */
int bqc_shard_fasta_span(bqc_ctx* ctx, int32_t span[2]); /* first / last FASTA position of the triplet-eligible reads so far (-1: none); waits for the batches in flight */
uint64_t bqc_shard_state_bytes(const bqc_ctx* ctx);
int bqc_shard_resolve(bqc_ctx* ctx, const void* predecessor_state);
int bqc_shard_export(bqc_ctx* ctx, void* state);

/* Flat state vector (uint64 words, pure sums => additive across shards).
 * export/import take DEVICE pointers (e.g. a torch tensor's data_ptr) so a
 * caller can reduce them with RCCL between the two calls.
 * Behind the per-lane counters lie the k-mer sketches, [lane][pair = qi * n_k + ki], each
 * [sumCount][F2 table, F2size words][32 levels x R counters], a counter exported as min(15, count) in a 16-bit field, four
 * per word, counter j of level w in field w * R + j (F2size and R follow from sketch.e: 32768 and 524288 at 0.01, so
 * 1 + F2size + 8 R = 4227073 words per sketch).  The import takes the SUM of exported vectors and uses min(15, sum) per
 * counter, which is what one context counts over all the reads; a field holds 4369 x 15, so the sum of more than 4369
 * exported vectors is outside the contract.  Behind the sketches: the optional modules (below). */
uint64_t bqc_state_words(const bqc_ctx* ctx);
int bqc_state_export(bqc_ctx* ctx, void* dev_dst_u64);
int bqc_state_import(bqc_ctx* ctx, const void* dev_src_u64);
int bqc_state_export_host(bqc_ctx* ctx, uint64_t* host_dst);
int bqc_state_import_host(bqc_ctx* ctx, const uint64_t* host_src);

/* bqc_flush + finalisation (lengths, soft-clip prefix sums, empty-lane coverage
 * rule, sketch estimators).  The returned structure is owned by the context and
 * valid until the next finalize/destroy. */
int bqc_finalize(bqc_ctx* ctx, const bqc_counts** out);

/* Timing of the last bqc_process call measured with HIP events on the
 * library's own stream: total and per kernel (ms).  names/ms arrays are owned by ctx. */
int bqc_last_timing(bqc_ctx* ctx, uint32_t* n, const char* const** names, const float** ms);
int bqc_set_timing(bqc_ctx* ctx, int enable);

/* ---- `.bamqc` text (replaces writeOutput, bamqualcheck.cpp:156-233) -------- */
typedef struct bqc_header_info {
    const char* sample_id;          /* SM of the last @RG                                   */
    uint32_t n_names;               /* lane names in output order (lexicographic by ID)     */
    const char* const* lane_names;
    const uint32_t* lane_index;     /* index into counts->lanes for each name               */
} bqc_header_info;
int bqc_write_bamqc(const bqc_counts* counts, const bqc_header_info* hdr, const char* path);

/* ---- per-cycle base quality histograms (bqc_options.qual_by_cycle; not in the reference) -----------------------
 * H[lane][mate][cycle][q] = number of bases with Phred value q at sequencing cycle `cycle` (stored byte j of a read of length L is
 * cycle j, or L-1-j when 0x10 is set), over exactly the reads whose qualities enter qualcount: neither supplementary nor secondary,
 * 0x40 set -> mate 0, else 0x80 set -> mate 1, BQC_FLAG_NO_QUAL clear.  For every cycle: sum_q q * H[..][cycle][q] == qualcount[cycle].
 * Pure sums: the module's words lie behind the sketch's in the flat state vector, n_lanes x 2 x N x 224 of them (lane-major, then
 * mate, cycle, quality), and add across shards.
 *   n_cycles = min(N, the mate's n_cycles in bqc_mate_counts); n_q = 1 + the highest Phred value counted for the lane and mate (0: none)
 *   element [c][q] is hist[c * stride + q]
 * bqc_qual_by_cycle: valid after bqc_finalize; the view is owned by the context until the next finalize / destroy.  BQC_ERR_STATE:
 * the module is off, or nothing has been finalised; BQC_ERR_ARG: lane or mate out of range.
 * bqc_write_qual_by_cycle: the table as text, lanes in the order of `hdr` as in the `.bamqc`:
 *   sample_id <id> / lane <name> / base_qual_histogram_by_position_first <n_cycles> <n_q> / one line of n_q counts per cycle /
 *   base_qual_histogram_by_position_second <n_cycles> <n_q> / ... */
typedef struct bqc_qbc_view { uint32_t n_cycles, n_q, stride; const uint64_t* hist; } bqc_qbc_view;
int bqc_qual_by_cycle(bqc_ctx* ctx, uint32_t lane, uint32_t mate, bqc_qbc_view* out);
int bqc_write_qual_by_cycle(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path);

/* ---- mismatches by cycle and base quality (bqc_options.mismatch_by_cycle; not in the reference) -----------------
 * Two tables per read group and mate, for a capacity N:
 *   A[lane][mate][cycle][q]  bases that were compared with the genome        M[lane][mate][cycle][q]  those of them that differ from it
 * A read is counted iff  flag & 0x900 == 0;  a mate flag is set (0x40 -> mate 0, else 0x80 -> mate 1);  BQC_FLAG_NO_QUAL is clear;
 * flag & 0x4 is clear;  0 <= rid < n_refs;  the contig rid has been given with bqc_set_reference;  n_cigar > 0.  No mapq or AS filter;
 * duplicates and QC-fail reads count.
 * The walk, in BAM orientation and 64-bit signed arithmetic: j = 0 (stored base index), r = pos (genome position); for each CIGAR
 * operation of length n:  M, =, X (0, 7, 8): examine the pairs (j+t, r+t), t < n, then j += n, r += n;  I, S (1, 4): j += n;
 * D, N (2, 3): r += n;  H, P and any code of 9 or more: nothing.  `=` and `X` are compared by their bases, not believed.
 * A pair (jj, rr) is counted iff  jj < l_seq;  0 <= rr < the contig's length;  the read's 4-bit code is A, C, G or T (1, 2, 4, 8);
 * the genome's Dna5 code is 3 or less;  the quality byte q is 222 or less;  the cycle c = jj (l_seq-1-jj when 0x10 is set) is below N.
 * Hard clips do not shift cycles.  For a counted pair A[c][q] += 1, and M[c][q] += 1 if the read's base is not the genome's; a read
 * base N, = or any ambiguity code, and a genome N, enter neither table.
 * Pure sums: the module's words are [n_lanes][2 mates][2 tables: A then M][N][224] u64; they lie behind the sketch's words and IN
 * FRONT OF qual_by_cycle's in the flat state vector, and add across shards.
 *   n_cycles = min(N, the mate's n_cycles in bqc_mate_counts); n_q = 1 + the highest q with a non-zero A for the lane and mate (0: none)
 *   element [c][q] is aligned[c * stride + q] / mismatch[c * stride + q]
 * bqc_mismatch_by_cycle: valid after bqc_finalize; the view is owned by the context until the next finalize / destroy.  BQC_ERR_STATE:
 * the module is off, or nothing has been finalised; BQC_ERR_ARG: lane or mate out of range.
 * bqc_write_mismatch_by_cycle: the tables as text, lanes in the order of `hdr` as in the `.bamqc`:
 *   sample_id <id> / lane <name> / aligned_bases_by_position_and_qual_first <n_cycles> <n_q> / one line of n_q counts per cycle /
 *   mismatches_by_position_and_qual_first <n_cycles> <n_q> / ... / aligned_bases_by_position_and_qual_second ... /
 *   mismatches_by_position_and_qual_second ...
 * "The contig is on the card" is decided per batch at its launch.  The program uploads every contig of the FASTA file that is a BAM
 * reference before a batch with a read on it is submitted, in every mode but the non-default BQC_BG_REFS=1 (the uploader beside the
 * record loop), which is out of this module's scope. */
typedef struct bqc_mbc_view { uint32_t n_cycles, n_q, stride; const uint64_t* aligned; const uint64_t* mismatch; } bqc_mbc_view;
int bqc_mismatch_by_cycle(bqc_ctx* ctx, uint32_t lane, uint32_t mate, bqc_mbc_view* out);
int bqc_write_mismatch_by_cycle(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path);

/* ---- adapter content by cycle (bqc_modules.adapter_by_cycle through bqc_create_ex; not in the reference) --------------------------
 * Adapter set.  1 to 8 adapters.  Each has a name: 1 to 31 characters of [A-Za-z0-9_.-].  Each has a sequence: 8 to 16 letters of
 * ACGT, upper case.  Built-in set, used when none is given, in this order:
 *   Illumina_Universal AGATCGGAAGAG   Illumina_SmallRNA_3p TGGAATTCTCGG   Illumina_SmallRNA_5p GATCGTCGGACT
 *   Nextera_Transposase CTGTCTCTTATA  PolyA AAAAAAAAAAAA                  PolyG GGGGGGGGGGGG
 * Examined reads.  A read is examined when all of these hold:  flag & 0x900 == 0;  flag & 0xC0 != 0;  l_seq > 0;  lane < n_lanes.
 * The mate is 0 with 0x40, else 1 (k_qcyc's rule).  There is no quality, mapping or duplicate condition: BQC_FLAG_NO_QUAL reads and
 * unmapped reads are examined.
 * Orientation.  For an examined read of length L, the base of cycle c is: stored base c, for a forward read; the complement of stored
 * base L-1-c, when 0x10 is set.  Stored 4-bit codes 1, 2, 4 and 8 are A, C, G and T.  Every other code matches nothing: N, = and the
 * ambiguity codes.
 * Occurrence and first hit.  Adapter a of length m occurs at cycle c when both hold:  c + m <= L;  the bases of cycles c ... c+m-1
 * equal a letter for letter.  An adapter cut off by the end of the read does not occur.  Its first hit is the lowest such c.
 * Tables, for a capacity N:
 *   F[lane][mate][slot][c] counts the examined reads whose first hit of adapter `slot` is c.  A first hit at or behind N is not counted.
 *   E[lane][mate][min(L,N)-1] counts the examined reads by length.  This is what the fractions are taken of.
 * The fraction of reads with adapter a at or before cycle c is  sum F[a][0..c] / sum E[c..].
 * State.  All of it is pure sums.  The words are [n_lanes][2 mates][9 rows: slots 0...7, then E][N] u64.  They lie in the flat state
 * vector behind the sketch's words and IN FRONT OF mismatch_by_cycle's and qual_by_cycle's.  Unused slots stay zero.  With the module
 * off: no allocation, no launch, the same bqc_state_words.  With the module on: the `.bamqc`, `.qbc` and `.mbc` are the same bytes as
 * without it.
 *   n_cycles = 1 + the highest index with a non-zero E for the lane and mate, 0 when there is none (from the module's own sums, not
 *   from bqc_mate_counts);  n_adapters, adapters: the set in use;  element [a][c] is first_hit[a * stride + c], [c] reads_by_length[c]
 * bqc_adapter_by_cycle: valid after bqc_finalize; the view is owned by the context until the next finalize / destroy.  BQC_ERR_STATE:
 * the module is off, or nothing has been finalised; BQC_ERR_ARG: lane or mate out of range.
 * bqc_write_adapter_by_cycle: the tables as text, lanes in the order of `hdr`, key-then-values lines as in the `.bamqc`:
 *   sample_id <id> / lane <name> / adapter_reads_by_length_first v0 ... v(n_cycles-1) /
 *   adapter_first_hit_by_position_first <name> <sequence> v0 ... v(n_cycles-1), one such line per adapter in the set's order /
 *   adapter_reads_by_length_second ... / adapter_first_hit_by_position_second <name> <sequence> ...
 * With n_cycles = 0 the key lines stand without values. */
typedef struct bqc_adp_view {
    uint32_t n_cycles, n_adapters, stride;
    const uint64_t* reads_by_length;   /* [c] */
    const uint64_t* first_hit;         /* [a * stride + c] */
    const bqc_adapter* adapters;       /* the set in use, n_adapters entries */
} bqc_adp_view;
int bqc_adapter_by_cycle(bqc_ctx* ctx, uint32_t lane, uint32_t mate, bqc_adp_view* out);
int bqc_write_adapter_by_cycle(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path);

/* ---- GC bias: genome windows and read starts by GC (bqc_enable_gc_bias; not in the reference) ------------------------------------
 * Window length W: 100 by default, 20 <= W <= 1000.  There are 101 bins, g = 0 ... 100.
 * GC bin of a window.  For a window [s, s+W) of contig rid, with 0 <= s and s + W <= len(rid):
 *   gc = number of bases with Dna5 code 1 or 2 (C, G);  n = number of bases with code 4 (N);
 *   if n > 4 the window has no bin;  otherwise g = floor(100 * gc / (W - n)).
 * Genome table G[g].  For every contig that has been given with bqc_set_reference (or moved in with bqc_move_references), every s in
 * [0, len - W] whose window has a bin adds 1 to G[g].  A contig shorter than W adds nothing.  G belongs to the genome, not to the
 * reads: it is not part of the state vector, it is not summed by import or the reduce, and bqc_reset does not touch it.  The context
 * that finalises computes it at bqc_finalize from the contigs it holds at that moment, into a buffer of its own.
 * Which reads count.  A read is examined iff all of these hold:  flag & 0x904 == 0 (primary and mapped);  n_cigar > 0;
 * 0 <= rid < n_refs and the contig is on the card.  There is no mate-flag requirement, so single-end reads count.  There is no
 * mapping-quality filter.  Duplicates and QC-fail reads count, as in the `.qbc` and `.mbc`.  A read group at or behind n_lanes cannot
 * reach the kernel: the pre-pass refuses such a batch.
 * A read's window.  Positions are 0-based and the arithmetic is 64-bit signed.  Forward read (0x10 clear): s = pos.  Reverse read:
 * s = end - W, where end = pos + the sum of the lengths of the CIGAR operations M, D, N, =, X (0, 2, 3, 7, 8).  The read is counted iff
 * 0 <= s, s + W <= len(rid), and the window has a bin g.  The read's own length plays no part: a read shorter than W still has a
 * window of W genome bases.
 * Read tables, per read group.  R[lane][g] += 1 for every counted read.  For a counted read without BQC_FLAG_NO_QUAL:
 * B[lane][g] += l_seq;  Q[lane][g] += the sum of its quality bytes as stored, each 0 ... 255.  A counted read without qualities
 * enters R only.
 * What a consumer derives:  normalised coverage of bin g = (R[g] / sum R) / (G[g] / sum G);  mean base quality at GC g = Q[g] / B[g].
 * bqc_enable_gc_bias switches the module on, after creation (bqc_options and bqc_modules stay as they are).  BQC_ERR_ARG, with a
 * message that names the value: a window outside 20 ... 1000.  BQC_ERR_STATE: a second call; a call after the context has taken a
 * batch (bqc_submit, bqc_submit_async, bqc_upload, bqc_anchor_enqueue / bqc_submit_anchored), has exported or imported state, or has
 * been finalised.  The call allocates the tables: after it bqc_state_words is larger by n_lanes * 3 * 101 words, [n_lanes][3 rows: R,
 * B, Q][101] u64 without padding, behind the sketch's words (and indel_by_cycle's, below) and IN FRONT OF adapter_by_cycle's,
 * mismatch_by_cycle's and qual_by_cycle's.  All of them are pure sums: export / import, bqc_reset, shard hand-over and the reduce treat them as the other words.
 * Two contexts exchange state only when both or neither have the module on (their bqc_state_words differ otherwise).  Without the
 * call: no allocation, no launch, the same bqc_state_words and the same offsets.  With it: the `.bamqc`, `.qbc`, `.mbc` and `.adp` are
 * the same bytes as without it.
 * bqc_gc_bias: valid after bqc_finalize; the view (n_bins = 101 entries per array) is owned by the context until the next finalize /
 * destroy.  BQC_ERR_STATE: the module is off, or nothing has been finalised; BQC_ERR_ARG: lane out of range.
 * bqc_write_gc_bias: the tables as text, lanes in the order of `hdr`, key-then-values lines as in the `.bamqc`:
 *   sample_id <id> / lane <name> / gc_bias_window <W> / genome_windows_by_gc v0 ... v100 / read_starts_by_gc v0 ... v100 /
 *   bases_by_gc v0 ... v100 / base_qual_sum_by_gc v0 ... v100 */
int bqc_enable_gc_bias(bqc_ctx* ctx, uint32_t window);   /* 20 <= window <= 1000 */
typedef struct bqc_gcb_view {
    uint32_t window, n_bins;
    const uint64_t *genome_windows, *read_starts, *bases, *qual_sum;
} bqc_gcb_view;
int bqc_gc_bias(bqc_ctx* ctx, uint32_t lane, bqc_gcb_view* out);   /* after bqc_finalize; n_bins = 101 */
int bqc_write_gc_bias(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path);

/* ---- indels by cycle and by length (bqc_enable_indel_by_cycle; not in the reference) ----------------------------------------------
 * What the `.mbc` leaves out: where in the read insertions and deletions occur, and how long they are (samtools stats: IC and ID).
 * Capacity N: 1 <= N <= max_read_len.  Length bins: K = 64.
 * Examined reads.  A read is examined when all of these hold:  flag & 0x900 == 0;  flag & 0xC0 != 0;  flag & 0x4 is clear;
 * n_cigar > 0;  l_seq > 0;  lane < n_lanes.  The mate is 0 with 0x40, else 1 (k_qcyc's rule).  There is no condition on mapping
 * quality, on duplicates, on BQC_FLAG_NO_QUAL, on rid or on a loaded contig: the genome is not read.  A read group at or behind
 * n_lanes and a primary read without a mate flag cannot reach the kernel: the pre-pass refuses such a batch.
 * The walk, in stored (BAM) orientation and 64-bit arithmetic, for a read of L = l_seq bases: j = 0; for each CIGAR operation with code
 * op and length n, in stored order:
 *   M, =, X, S (0, 7, 8, 4):  j += n.
 *   I (1):  an insertion of n bases at stored index j.  It is an event iff n >= 1 and j + n <= L.  Its cycle is c = j for a forward
 *     read and c = L - j - n with 0x10 set: the first of the inserted bases in sequencing order.  Then j += n, event or not.
 *   D (2):  a deletion of n genome bases between stored bases j-1 and j.  It is an event iff n >= 1 and 0 < j < L: a read base on both
 *     sides.  Its cycle is the last cycle sequenced before the gap: c = j - 1 for a forward read, c = L - 1 - j with 0x10 set.
 *     j is unchanged.
 *   N, H, P (3, 5, 6) and every code of 9 or more:  nothing.  A reference skip is not a deletion.  Hard clips do not shift cycles.
 * An event whose cycle is at or behind N enters NO table, the length tables included.
 * Tables, per read group and mate:
 *   E[min(L, N) - 1] += 1 for every examined read (the denominator);
 *   IC[c] += 1 and IL[min(n, K) - 1] += 1 for an insertion event;  DC[c] += 1 and DL[min(n, K) - 1] += 1 for a deletion event.
 * The last bin of a length table holds every length of K or more.  By construction sum IC = sum IL and sum DC = sum DL.  The insertion
 * rate at cycle c is IC[c] / sum E[c..].
 * State.  All of it is pure sums.  The words of a read group and mate are [3 rows: E, IC, DC][N] followed by [2 rows: IL, DL][64],
 * all u64 without padding; in full [n_lanes][2 mates] of that, n_lanes * 2 * (3 N + 128) words.  They lie behind the sketch's
 * words (and the substitutions', below), IN FRONT OF gc-bias's, adapter_by_cycle's, mismatch_by_cycle's and qual_by_cycle's.  Export / import, bqc_reset, shard
 * hand-over and the reduce treat them as the other words, so the module works across shards (--gpus N), unlike the GC bias.  Two
 * contexts exchange state only when both or neither have the module on, with the same N.
 * bqc_enable_indel_by_cycle switches the module on, after creation (bqc_options and bqc_modules stay as they are).  BQC_ERR_ARG, with
 * a message that names the value: N = 0 or N > max_read_len.  BQC_ERR_STATE: a second call; a call after the context has taken a batch,
 * has exported or imported state, or has been finalised (bqc_enable_gc_bias's conditions).  Both enable calls may be made on one
 * context, in either order, with the same layout.  Without the call: no allocation, no launch, the same bqc_state_words and the same
 * offsets.  With it: the `.bamqc`, `.qbc`, `.mbc`, `.adp` and `.gcb` are the same bytes as without it.
 * bqc_indel_by_cycle: valid after bqc_finalize; the view is owned by the context until the next finalize / destroy.
 *   n_cycles = 1 + the highest index with a non-zero E for the lane and mate, 0 when there is none (from the module's own sums, as in
 *   the `.adp`): the entries of reads_by_length, insertions and deletions.  n_len = 64: the entries of the two length arrays, entry
 *   i for length i + 1.
 * BQC_ERR_STATE: the module is off, or nothing has been finalised; BQC_ERR_ARG: lane or mate out of range.
 * bqc_write_indel_by_cycle: the tables as text, lanes in the order of `hdr`, key-then-values lines as in the `.bamqc`:
 *   sample_id <id> / lane <name> / indel_reads_by_length_first v0 ... v(n_cycles-1) / insertions_by_position_first v0 ... /
 *   deletions_by_position_first v0 ... / insertion_length_histogram_first v1 ... v64 / deletion_length_histogram_first v1 ... v64 /
 *   the same five lines with _second.
 * With n_cycles = 0 the three per-position keys stand without values; the two length lines always have 64 values. */
int bqc_enable_indel_by_cycle(bqc_ctx* ctx, uint32_t n_cycles);   /* 1 <= n_cycles <= max_read_len */
typedef struct bqc_ibc_view {
    uint32_t n_cycles, n_len;
    const uint64_t *reads_by_length, *insertions, *deletions, *insertion_lengths, *deletion_lengths;
} bqc_ibc_view;
int bqc_indel_by_cycle(bqc_ctx* ctx, uint32_t lane, uint32_t mate, bqc_ibc_view* out);   /* after bqc_finalize; n_len = 64 */
int bqc_write_indel_by_cycle(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path);

/* ---- substitutions by sequence context and by cycle (bqc_enable_substitutions; not in the reference) -------------------------------
 * What the `.mbc` leaves out: which base became which, and in what sequence context — the two tables that Picard's
 * CollectSequencingArtifactMetrics, mapDamage's position curves and the 96-class substitution spectrum are folds of.
 * Parameters.  Cycle capacity N, 1 <= N <= max_read_len.  Minimum base quality Q, 0 <= Q <= 222.  Minimum mapping quality MQ,
 * 0 <= MQ <= 255; mapq is compared as a plain number, 255 is not special.  (The program's defaults: 1024, 20 and 30, the two last
 * Picard's.)
 * Examined reads.  mismatch_by_cycle's conditions exactly:  flag & 0x900 == 0;  a mate flag is set (0x40: mate 0, else 0x80: mate 1);
 * BQC_FLAG_NO_QUAL is clear;  flag & 0x4 is clear;  l_seq > 0;  n_cigar > 0;  lane < n_lanes;  0 <= rid < n_refs and the contig is on
 * the card (mismatch_by_cycle's meaning, and its BQC_BG_REFS=1 exclusion).  In addition mapq >= MQ.  Duplicates and QC-fail reads count.
 * The walk is mismatch_by_cycle's, word for word: 64-bit signed arithmetic, j = 0 and r = pos;  M, =, X examine the pairs
 * (j + t, r + t), t < n, and advance both;  I and S advance j;  D and N advance r;  H, P and every code of 9 or more do nothing.
 * Examined pairs.  A pair (jj, rr) is examined iff all of these hold:  jj < l_seq;  0 <= rr < the contig's length;  the read's 4-bit
 * code is 1, 2, 4 or 8;  the genome's Dna5 code g[rr] <= 3;  the quality byte q has Q <= q <= 222;  the cycle c < N, where c = jj, or
 * l_seq - 1 - jj with 0x10 set.
 * Orientation: as sequenced.  b = the read base as a code 0..3 (A, C, G, T), t = g[rr].  Forward read: b' = b, t' = t.  With 0x10
 * set: b' = 3 - b, t' = 3 - t.  The strand index is s = (flag >> 4) & 1.
 * Table Y, by cycle.  For every examined pair  Y[lane][mate][c][t'][b'] += 1:  sixteen bins a cycle.
 * Table X, by context.  An examined pair enters X iff  1 <= rr  and  rr + 1 < the contig's length  and  g[rr-1] <= 3  and
 * g[rr+1] <= 3.  The context as sequenced:  forward read  ctx = 16 g[rr-1] + 4 t + g[rr+1];  reverse read
 * ctx = 16 (3 - g[rr+1]) + 4 (3 - t) + (3 - g[rr-1]).  Then  X[lane][mate][s][ctx][b'] += 1.
 * The neighbours are GENOME bases: a run of one position, a base beside an insertion, a clip or a deletion has a context all the
 * same, and the neighbour may lie outside the alignment.  By construction sum X <= sum Y per lane and mate; the difference is the
 * examined pairs with a missing or N neighbour.
 * State.  All of it is pure sums.  The words of a read group and mate are X [2 strands][64][4] then Y [N][16], u64 without padding:
 * 512 + 16 N words; in full n_lanes * 2 * (512 + 16 N).  They lie directly behind the sketch's words, IN FRONT OF indel_by_cycle's,
 * gc-bias's, adapter_by_cycle's, mismatch_by_cycle's and qual_by_cycle's: every other module's distance from the end of the vector
 * stays what it is.  Export / import, bqc_reset, shard hand-over and the reduce treat them as the other words (--gpus N works).  Two
 * contexts exchange state only when both or neither have the module on, with the same N (their bqc_state_words differ otherwise).
 * bqc_enable_substitutions switches the module on, after creation (bqc_options and bqc_modules stay as they are; the ABI version
 * stays 2).  BQC_ERR_ARG, with a message that names the value: N = 0, N > max_read_len, Q > 222, MQ > 255.  BQC_ERR_STATE: a second
 * call; a call after the context has taken a batch, has exported or imported state, or has been finalised (bqc_enable_gc_bias's
 * conditions).  The three enable calls may be made on one context in any order, with the same layout.  Without the call: no
 * allocation, no launch, the same bqc_state_words and the same offsets.  With it: the `.bamqc`, `.qbc`, `.mbc`, `.adp`, `.gcb` and
 * `.ibc` are the same bytes as without it.
 * bqc_substitutions: valid after bqc_finalize; the view is owned by the context until the next finalize / destroy.
 *   by_context: 512 entries, element [s][ctx][b'].  by_cycle: 16 n_cycles entries, element [c * 16 + t' * 4 + b'].
 *   n_cycles = 1 + the highest cycle with a non-zero bin of Y for the lane and mate, 0 when there is none.
 * BQC_ERR_STATE: the module is off, or nothing has been finalised; BQC_ERR_ARG: lane or mate out of range.
 * bqc_write_substitutions: the tables as text, lanes in the order of `hdr`, key-then-values lines as in the `.bamqc`:
 *   sample_id <id> / lane <name> / substitution_min_base_qual <Q> / substitution_min_mapq <MQ> /
 *   substitutions_by_context_first_forward <CTX> vA vC vG vT   (64 lines, CTX = AAA, AAC, ... TTT: the genome as sequenced; the
 *   values: the read base as sequenced) / substitutions_by_context_first_reverse <CTX> vA vC vG vT   (64 lines) /
 *   substitutions_by_position_first <n_cycles> 16 / one line of 16 counts per cycle (template A -> read A C G T, template C -> ...) /
 *   the same three blocks with _second. */
int bqc_enable_substitutions(bqc_ctx* ctx, uint32_t n_cycles, uint32_t min_base_qual, uint32_t min_mapq);
typedef struct bqc_sbc_view {
    uint32_t n_cycles, min_base_qual, min_mapq;
    const uint64_t *by_context, *by_cycle;
} bqc_sbc_view;
int bqc_substitutions(bqc_ctx* ctx, uint32_t lane, uint32_t mate, bqc_sbc_view* out);   /* after bqc_finalize */
int bqc_write_substitutions(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path);

/* ---- allele counts at given sites (bqc_enable_site_alleles; not in the reference) ---------------------------------------------------
 * The other tables describe the chemistry; this one describes the sample.  Per read group and per site of a given list it counts the
 * reads that show A, C, G and T there, by strand: the table that a fingerprint at known SNPs (Picard CheckFingerprint), the agreement
 * of read groups (a lane swap) and the minor-allele fraction at homozygous sites (contamination, VerifyBamID's input) are folds of.
 * Sites.  S sites (rid, pos), pos counted from 0, strictly increasing by (rid, pos);  0 <= rid < n_refs;  0 <= pos <= 2^31 - 2;
 * 1 <= S and n_lanes * S <= 2^24 (at most 1 GiB of counters).
 * Parameters.  Minimum base quality Q, 0 ... 222 (the program's default 20).  Minimum mapping quality MQ, 0 ... 255 (default 20); mapq
 * is compared as a plain number, 255 is not special.
 * Examined reads.  flag & 0xF04 == 0 (mapped, primary, not QC-fail, not a duplicate, not supplementary);  mapq >= MQ;  n_cigar > 0;
 * l_seq > 0;  BQC_FLAG_NO_QUAL is clear;  lane < n_lanes;  0 <= rid < n_refs.  The mate flags are not looked at.  The genome is NOT
 * read: no contig need be loaded.
 * The walk, in stored orientation and 64-bit arithmetic: j = 0, g = pos; for every CIGAR operation (op, n) in stored order
 *   M, =, X (0, 7, 8):  for every site (rid, p) with g <= p < g + n and i = j + (p - g) < l_seq take the read's 4-bit code at stored
 *     index i and the quality q = qual[i]; if the code is 1, 2, 4 or 8 (A, C, G, T: b = 0 ... 3) and Q <= q <= 222 then
 *     T[lane][site][4 s + b] += 1, where s = 1 with 0x10 set, else 0.  Then j += n and g += n.
 *   I, S (1, 4):  j += n.      D, N (2, 3):  g += n; a site under a deletion or a skip gets nothing.
 *   H, P and every code of 9 or more:  nothing.
 * Bases are counted in genome orientation, as a pileup shows them (a reverse read's stored bases are that already).  The code `=`
 * (0), N and the ambiguity codes count nowhere.  g only grows, so a read adds at most 1 to a site.  Two mates that overlap on a site
 * BOTH count: read names are not on the card, and there is no overlap correction.
 * State.  [n_lanes][S][8] u64, pure sums, no padding: n_lanes * S * 8 words directly behind the sketch's words, IN FRONT OF the
 * substitutions' and every other module's: their distance from the end of the vector stays what it is.  Export / import, bqc_reset
 * (the table goes back to zero, the sites stay), shard hand-over and the reduce treat them as the other words (--gpus N works).  Two
 * contexts exchange state only when both have the module on with the same S (their bqc_state_words differ otherwise; the lists
 * themselves are not compared).
 * bqc_enable_site_alleles switches the module on, after creation, in any order with the other enable calls (bqc_options and
 * bqc_modules stay as they are; the ABI version stays 2); the list is copied.  BQC_ERR_ARG, with a message that names the value and,
 * for the list, the index of the first offending site: S = 0;  n_lanes * S > 2^24;  a rid or a pos out of range;  a site that does
 * not lie strictly behind its predecessor;  Q > 222;  MQ > 255.  BQC_ERR_STATE: a second call; a call after the context has taken a
 * batch, has exported or imported state, or has been finalised (bqc_enable_gc_bias's conditions).  Without the call: no allocation,
 * no launch, the same bqc_state_words and the same offsets.  With it: every other output is the same bytes as without it.
 * bqc_site_alleles: valid after bqc_finalize; the view is owned by the context until the next finalize / destroy.  rid and pos: the
 * list as given; counts: S x 8 entries, element [site * 8 + 4 s + b].  BQC_ERR_STATE: the module is off, or nothing has been
 * finalised; BQC_ERR_ARG: lane out of range.
 * bqc_write_site_alleles: the table as text, lanes in the order of `hdr`, key-then-values lines as in the `.bamqc`.  bqc_header_info
 * carries no contig names, hence ref_names[n_refs] (BQC_ERR_ARG when a site's contig has none):
 *   sample_id <id> / lane <name> / site_allele_min_base_qual <Q> / site_allele_min_mapq <MQ> / site_alleles <S> /
 *   <contig> <pos, counted from 1> fA fC fG fT rA rC rG rT     (one line per site, in the table's order) */
int bqc_enable_site_alleles(bqc_ctx* ctx, uint32_t n_sites, const int32_t* rid, const int32_t* pos, uint32_t min_base_qual, uint32_t min_mapq);
typedef struct bqc_sac_view {
    uint32_t n_sites, min_base_qual, min_mapq;
    const int32_t *rid, *pos;
    const uint64_t* counts;
} bqc_sac_view;
int bqc_site_alleles(bqc_ctx* ctx, uint32_t lane, bqc_sac_view* out);   /* after bqc_finalize */
int bqc_write_site_alleles(bqc_ctx* ctx, const bqc_header_info* hdr, const char* const* ref_names, uint32_t n_refs, const char* path);

/* ---- depth over given regions (bqc_enable_region_coverage; not in the reference) ---------------------------------------------------
 * What an exome, a gene panel or an amplicon run is judged by: how much of the sequencing landed on the targets, how deep each target
 * is, which targets fall below a depth (Picard CollectHsMetrics, mosdepth --by).  For a whole genome: the window histogram (poscov), and the
 * depth in fixed genome windows (bqc_enable_window_depth, below).
 * Regions.  R regions (rid, start, end), counted from 0 and half-open;  0 <= rid < n_refs;  0 <= start < end <= 2^31 - 1;  sorted by
 * (rid, start) and disjoint: within a contig start[k] >= end[k-1] (abutting regions are allowed).  len[k] = end - start, B = sum of
 * len.  Region k owns len[k] + 1 slots from off[k] = sum over i < k of (len[i] + 1); the extra slot closes the region.  1 <= R and
 * n_lanes * (B + R + 4) <= 2^28 (2 GiB of words): a whole genome as "regions" is refused.
 * Parameters.  Minimum mapping quality MQ, 0 ... 255 (the program's default 20), compared as a plain number.  For finalize only, and
 * not part of the state: up to 8 depth thresholds, strictly increasing, each 1 ... 2^32 - 1 (n_thresholds = 0: 1, 10, 20, 30, 50,
 * 100), and a histogram cap D, 1 ... 16383 (the program's default 1000).
 * Examined reads.  flag & 0xF04 == 0;  mapq >= MQ;  n_cigar > 0;  l_seq > 0;  lane < n_lanes;  0 <= rid < n_refs.
 * BQC_FLAG_NO_QUAL is NOT looked at: no base or quality is read, only the CIGAR.  The mate flags are not looked at; two mates that
 * overlap BOTH count, as in the site alleles.  The genome is not read.
 * The walk, in stored order and 64-bit arithmetic: j = 0, g = pos, hit = false; for every CIGAR operation (op, n)
 *   M, =, X (0, 7, 8):  m = min(n, max(0, l_seq - j)); the positions [g, g + m) are covered;  A[lane] += m;  for every region of the
 *     read's contig with start < g + m and end > g:  lo = max(g, start), hi = min(g + m, end),
 *     Diff[lane][off + lo - start] += 1, Diff[lane][off + hi - start] -= 1 (modulo 2^64), hit = true.  Then j += n and g += n.
 *   I, S (1, 4):  j += n.      D, N (2, 3):  g += n; a deletion or a skip covers nothing (the .mbc / .sac convention, not mosdepth's).
 *   H, P and every code of 9 or more:  nothing.
 * Per read E[lane] += 1, and T[lane] += 1 when hit.
 * State.  Per lane [E, T, A, 0][B + R difference words], u64, pure sums modulo 2^64: n_lanes * (4 + B + R) words directly behind the
 * sketch's words, IN FRONT OF the site alleles' and every other module's: their distance from the end of the vector stays what it
 * is.  A region's len + 1 slots always sum to 0, so a plain prefix sum over a lane's difference words is the depth inside every
 * region and 0 on every closing slot.  Export / import, bqc_reset (the words go back to zero, the regions stay), shard hand-over and
 * the reduce treat the words as the other words (--gpus N works).  Two contexts exchange state only when both have the module on with
 * the same B + R (the lists themselves are not compared; see bqc_finalize below).
 * Finalize products, per lane.  Per region: sum, min and max of the depth over its len positions and, per threshold t, the number of
 * positions of depth >= t.  Over all B positions: the histogram H[0 ... D] (bin D: depth >= D).  bases_on_target = the sum of the
 * regions' sums.  The state is left as it is: finalize can be called again, and an export after it still gives difference words.
 * bqc_finalize fails with BQC_ERR_STATE and names the first such region when a closing slot's prefix is not 0: the words are not a
 * difference array of this list (an import from a context with another list of the same B + R).
 * bqc_enable_region_coverage switches the module on, after creation, in any order with the other enable calls (the ABI version stays
 * 2); the lists are copied.  BQC_ERR_ARG, with a message that names the value and, for the list, the index of the first offending
 * region, in this order: R = 0;  a null list;  MQ > 255;  more than 8 thresholds, a threshold out of range or not above its
 * predecessor;  D out of range;  a rid out of range, a start below 0, an end not behind its start, a region that begins in front of
 * its predecessor's end;  n_lanes * (B + R + 4) > 2^28.  BQC_ERR_STATE: a second call; a call after the context has taken a batch, has
 * exported or imported state, or has been finalised.  Without the call: no allocation, no launch, the same bqc_state_words and the
 * same offsets.  With it: every other output is the same bytes as without it.
 * bqc_region_coverage: valid after bqc_finalize; the view is owned by the context until the next finalize / destroy.  regions:
 * R x (3 + n_thresholds) entries, a region's sum, min, max, then its counts by threshold.  BQC_ERR_STATE: the module is off, or
 * nothing has been finalised; BQC_ERR_ARG: lane out of range.
 * bqc_write_region_coverage: the text, lanes in the order of `hdr`, key-then-values lines (BQC_ERR_ARG when a region's contig has no
 * name):
 *   sample_id <id> / lane <name> / region_min_mapq <MQ> / region_reads_examined <E> / region_reads_on_target <T> /
 *   region_aligned_bases <A> / region_bases_on_target <sum of sums> / region_target_bases <B> / region_depth_thresholds t1 ... tn /
 *   region_depth_histogram <D + 1> v0 ... vD / regions <R> /
 *   <contig> <start> <end> <sum> <min> <max> <ge_t1> ... <ge_tn>     (one line per region, BED coordinates, the list's order) */
int bqc_enable_region_coverage(bqc_ctx* ctx, uint32_t n_regions, const int32_t* rid, const int32_t* start, const int32_t* end, uint32_t min_mapq,
                               uint32_t n_thresholds, const uint64_t* thresholds, uint32_t depth_cap);
typedef struct bqc_rcv_view {
    uint32_t n_regions, min_mapq, n_thresholds, depth_cap;
    const int32_t *rid, *start, *end;
    uint64_t reads_examined, reads_on_target, aligned_bases, bases_on_target, target_bases;
    const uint64_t* thresholds; /* [n_thresholds] */
    const uint64_t* regions;    /* [n_regions][3 + n_thresholds] */
    const uint64_t* hist;       /* [depth_cap + 1] */
} bqc_rcv_view;
int bqc_region_coverage(bqc_ctx* ctx, uint32_t lane, bqc_rcv_view* out);   /* after bqc_finalize */
int bqc_write_region_coverage(bqc_ctx* ctx, const bqc_header_info* hdr, const char* const* ref_names, uint32_t n_refs, const char* path);

/* ---- duplicate sets by alignment signature (bqc_enable_duplicate_sets; not in the reference) ---------------------------------------
 * How much of the library is PCR duplicates and how large the library is (Picard MarkDuplicates / EstimateLibraryComplexity, FastQC's
 * duplication levels), computed from the alignments themselves and not from flag 0x400, which only repeats what an upstream tool
 * wrote (BQC_S_DUPLICATES).  Read names and the mate's position are not looked at.
 * Examined reads.  flag & 0xB04 == 0 (mapped, primary, not supplementary, not QC-fail);  n_cigar > 0;  l_seq > 0;  0 <= rid < n_refs;
 * lane < n_lanes.  Mapping quality, BQC_FLAG_NO_QUAL, the mate flags 0x40 / 0x80 and 0x400 are NOT conditions.  The genome is not read.
 * Class.  pair: 0x1 set, 0x8 clear, tlen > 0 (the leftmost end; it stands for its fragment).  second end: 0x1 set, 0x8 clear,
 * tlen < 0: counted in a scalar and otherwise left out (its fragment is its mate's).  single: every other examined read (unpaired,
 * the mate unmapped, tlen == 0).
 * Unclipped 5' position u5, 64-bit signed arithmetic over the CIGAR in stored order: lead = the sum of the lengths of the maximal
 * prefix of operations with code 4 or 5 (S, H); trail = the same for the maximal suffix, 0 when the prefix took every operation;
 * reflen = the sum over M, D, N, =, X (0, 2, 3, 7, 8).  Forward read (0x10 clear): u5 = pos - lead.  Reverse read: u5 = pos + reflen -
 * 1 + trail.  |u5| < 2^45 follows (at most 65 535 operations of fewer than 2^28 bases).
 * Signature.  (class, strand = flag >> 4 & 1, mate strand = flag >> 5 & 1 for class pair else 0, rid, u5, tlen for class pair else 0).
 * The read group is NOT part of it: a duplicate is a property of the library, and a library is spread over lanes.  Two reads are in one
 * SET iff their signatures are equal; this is exact.  As two words: k0 = (u5 + 2^45) | class << 46 | strand << 47 | mate strand << 48
 * (class: 0 single, 1 pair), k1 = rid | (uint32) tlen << 32.
 * Products.  Per read group, pure sums: E_single, E_pair (examined reads of the class), F_single, F_pair (those of them with 0x400
 * set), second_end.  Per context, over all read groups, for class c: U_c = the number of sets, largest_c = the reads of the largest
 * set, H_c[i], i = 1 ... 256 = the sets of i reads (bin 256: 256 and more).  sum over lanes of E_c = sum over sets of their reads.  The
 * observed duplicates of a class are sum E_c - U_c, to be set against sum F_c.
 * Estimated library size, from class pair, Picard's estimateLibrarySize in double precision: n = sum E_pair, c = U_pair; c = 0 or
 * c >= n: 0; otherwise f(x) = c / x - 1 + exp(-n / x);  m = 1, M = 100, while f(M c) > 0: M *= 10;  40 times: r = (m + M) / 2,
 * u = f(r c), u == 0: stop, u > 0: m = r, else M = r;  the estimate is (uint64) (c (m + M) / 2).
 * State.  A hash table in device memory, 24 bytes a slot, C = the smallest power of two >= 2 capacity (and >= 32) slots, and the
 * per-lane sums.  NONE of it is part of the flat state vector (as the GC bias's genome table): bqc_state_words and every offset are
 * the same with the module on, export and import carry none of it, shards cannot be merged (a set may have members in two shards:
 * --gpus N is refused by the program).  bqc_reset empties the table and the sums and keeps the allocation.
 * Overflow.  When the reads hold more than `capacity` different signatures (both classes together) the stream fails with
 * BQC_ERR_RANGE where other errors found on the card surface (a later submit, sync, flush or finalize); the message names the
 * capacity and --duplicate-sets-capacity.
 * bqc_enable_duplicate_sets switches the module on, after creation, in any order with the other enable calls (the ABI version stays
 * 2).  BQC_ERR_ARG, the message names the value: capacity outside 16 ... 2^31.  BQC_ERR_STATE: a second call; a call after the
 * context has taken a batch, has exported or imported state, or has been finalised.  Without the call: no allocation, no launch.
 * With it: every other output is the same bytes as without it.
 * bqc_duplicate_sets: valid after bqc_finalize (which leaves the table as it is: it may be called again); the view is owned by the
 * context until the next finalize / destroy.  BQC_ERR_STATE: the module is off, or nothing has been finalised.
 * bqc_write_duplicate_sets: the text, lanes in the order of `hdr`, key-then-values lines:
 *   sample_id <id> / duplicate_sets_capacity <capacity> /
 *   lane <name> / duplicate_reads_examined_single <E> / duplicate_reads_examined_pair <E> / duplicate_reads_flagged_single <F> /
 *   duplicate_reads_flagged_pair <F> / duplicate_reads_second_end <n>                                   (these six per read group)
 *   all_lanes / duplicate_sets_single <U> / duplicate_sets_pair <U> / duplicate_set_largest_single <n> / duplicate_set_largest_pair <n> /
 *   duplicate_set_size_histogram_single v1 ... v256 / duplicate_set_size_histogram_pair v1 ... v256 /
 *   duplicate_estimated_library_size <L> */
int bqc_enable_duplicate_sets(bqc_ctx* ctx, uint64_t capacity);
typedef struct bqc_dup_view {
    uint64_t capacity;
    uint32_t n_lanes, pad;
    uint64_t sets[2], largest[2];   /* [class: 0 single, 1 pair] */
    const uint64_t* hist[2];        /* [256]: sets of 1 ... 255 reads, of 256 and more */
    uint64_t estimated_library_size;
    const uint64_t* lanes;          /* [n_lanes][5]: E_single, E_pair, F_single, F_pair, second_end */
} bqc_dup_view;
int bqc_duplicate_sets(bqc_ctx* ctx, bqc_dup_view* out);   /* after bqc_finalize */
int bqc_write_duplicate_sets(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path);

/* ---- depth in fixed genome windows (bqc_enable_window_depth; not in the reference) -------------------------------------------------
 * What a whole-genome run is judged by: where the depth is (mosdepth --by 1000, samtools idxstats, the input of read-depth CNV
 * callers).  The X : autosome and Y : autosome ratios, a chromosome at 1.5 x or 0.5 x of the median, the share of reads on chrM or
 * decoys, the spread of the window depths and the low-mapping-quality depth beside the usable depth are folds of it.
 * Windows.  W is the window size, 100 <= W <= 2^24 (the program's default 1000).  Contig rid of length len[rid] (>= 0; BAM stores it
 * in 31 bits) has nw[rid] = ceil(len / W) windows, none when len is 0; window k is [k W, min((k + 1) W, len)).  woff[rid] is the
 * running sum of nw[], NW = woff[n_refs].  n_lanes * (4 + 3 NW) <= 2^28 (2 GiB of words).
 * Parameter.  Minimum mapping quality MQ, 0 ... 255 (the program's default 20), compared as a plain number: a read is of class GOOD
 * when mapq >= MQ, otherwise LOW.
 * Examined reads.  flag & 0xF04 == 0;  n_cigar > 0;  l_seq > 0;  lane < n_lanes;  0 <= rid < n_refs — the region coverage's
 * conditions without the one on mapq.  BQC_FLAG_NO_QUAL and the mate flags are not looked at; two mates that overlap BOTH count.  The
 * genome is not read, nor any base or quality.
 * The walk, in stored order and 64-bit arithmetic: j = 0, g = pos; for every CIGAR operation (op, n)
 *   M, =, X (0, 7, 8):  m = min(n, max(0, l_seq - j)); the positions [g, g + m) are covered.  A covered position p with
 *     0 <= p < len[rid] belongs to window floor(p / W) of the contig and adds 1 to that window's word of the read's class, bases or
 *     bases_low; every other covered position adds 1 to X[lane].  Then j += n and g += n.
 *   I, S (1, 4):  j += n.      D, N (2, 3):  g += n; a deletion or a skip covers nothing.
 *   H, P and every code of 9 or more:  nothing.
 * Per read E[lane] += 1 (good) or E_low[lane] += 1 (low); a good read with 0 <= pos < len[rid] adds 1 to reads[floor(pos / W)] of
 * its contig, any other read to no `reads` word.
 * State.  Per lane [E, E_low, X, 0][reads NW][bases NW][bases_low NW], u64, pure sums modulo 2^64: n_lanes * (4 + 3 NW) words directly
 * behind the sketch's words, IN FRONT OF the region coverage's and every other module's: their distance from the end of the vector
 * stays what it is.  Export / import, bqc_reset (the words go back to zero, the tables stay), shard hand-over and the reduce treat the
 * words as the other words (--gpus N works).  Two contexts exchange state only when both have the module on with the same NW.
 * Finalize products, per lane, made on the host from a copy of the words: per contig the sums of reads, bases and bases_low over its
 * windows; a histogram of floor(bases[w] / length(w)) with 1001 bins, the last open, over the windows of the contigs whose main_chrom
 * entry is 1.  The state is left as it is: finalize can be called again and gives the same views.
 * bqc_enable_window_depth switches the module on, after creation, in any order with the other enable calls (the ABI version stays
 * 2); ref_len holds the n_refs lengths of the context's contigs and is copied.  BQC_ERR_ARG, with a message that names the value, in
 * this order: W out of range;  MQ > 255;  a null list (n_refs > 0);  a negative length (with the contig's index);
 * n_lanes * (4 + 3 NW) > 2^28 (the message names NW, W and the number of read groups).  BQC_ERR_STATE: a second call; a call after
 * the context has taken a batch, has exported or imported state, or has been finalised.  Without the call: no allocation, no launch,
 * the same bqc_state_words and the same offsets.  With it: every other output is the same bytes as without it.
 * bqc_window_depth: valid after bqc_finalize; the view is owned by the context until the next finalize / destroy.  BQC_ERR_STATE: the
 * module is off, or nothing has been finalised; BQC_ERR_ARG: lane out of range.
 * bqc_write_window_depth: the text, lanes in the order of `hdr`, key-then-values lines (BQC_ERR_ARG when n_refs is not the
 * context's or a contig has no name):
 *   sample_id <id> / lane <name> / window_depth_window <W> / window_depth_min_mapq <MQ> / window_depth_reads_examined <E> /
 *   window_depth_reads_low_mapq <E_low> / window_depth_bases_outside_contigs <X> / window_depth_histogram 1001 v0 ... v1000 /
 *   contigs <n_refs> /
 *   <contig> <length> <windows> <reads> <bases> <bases_low_mapq>     (one line per contig, the header's order) /
 *   windows <lines that follow> <NW> /
 *   <contig> <start> <end> <reads> <bases> <bases_low_mapq>          (only windows with a word that is not 0, in order) */
#define BQC_WDP_HIST_BINS 1001
int bqc_enable_window_depth(bqc_ctx* ctx, uint32_t window, const int32_t* ref_len, uint32_t min_mapq);
typedef struct bqc_wdp_view {
    uint32_t window, min_mapq, n_windows, n_refs;
    const uint32_t* woff;      /* [n_refs + 1] */
    const uint32_t* ref_len;   /* [n_refs] */
    uint64_t reads_examined, reads_low_mapq, bases_outside;
    const uint64_t* reads;     /* [n_windows] */
    const uint64_t* bases;     /* [n_windows] */
    const uint64_t* bases_low; /* [n_windows] */
    const uint64_t* contigs;   /* [n_refs][3]: reads, bases, bases_low */
    const uint64_t* hist;      /* [1001] */
} bqc_wdp_view;
int bqc_window_depth(bqc_ctx* ctx, uint32_t lane, bqc_wdp_view* out);   /* after bqc_finalize */
int bqc_write_window_depth(bqc_ctx* ctx, const bqc_header_info* hdr, const char* const* ref_names, uint32_t n_refs, const char* path);

/* ---- overrepresented sequences and duplication by sequence (bqc_enable_overrepresented; not in the reference) -----------------------
 * Which read sequences occur far too often, and how duplicated the reads are AS SEQUENCES (FastQC's overrepresented sequences and
 * duplication levels, with exact counts): adapter dimers, rRNA and PhiX carry-over, primer artefacts, poly-G tails, amplicon
 * dominance.  It is the duplication measure that also works where the duplicate sets cannot: unaligned and unmapped reads.
 * Examined reads.  flag & 0x900 == 0;  flag & 0xC0 != 0;  l_seq > 0;  lane < n_lanes.  The mate is 0 with 0x40, else 1 (k_qcyc's
 * rule).  Unmapped reads, QC-fail reads, duplicates and BQC_FLAG_NO_QUAL reads are examined.  No quality, CIGAR, contig or genome is
 * read.
 * Key.  K is the prefix length, 20 ... 56 (the program's default 50), and n = min(l_seq, K).  The key is the first n bases AS
 * SEQUENCED, together with n and the mate: of a forward read the stored bases 0 ... n-1; of a reverse read (0x10) the stored bases
 * L-1 down to L-n, each complemented — a reverse read that stores revcomp(S) and a forward read that stores S have one key.  Two reads
 * are in one SET iff their keys are equal; the read group is NOT part of the key, as in the duplicate sets.  Reads that agree in the
 * first K bases and differ behind them are in one set; ACGT and ACGTA, with l_seq 4 and 5, are two sets.  If any of the n bases is not
 * A, C, G or T (stored codes 1, 2, 4, 8; the other twelve, N and = among them), the read is SKIPPED: counted per read group and mate,
 * and no part of any set.  (FastQC counts a poly-N read as a sequence; here a run of them shows up as `skipped`.)
 * Products.  Per read group, pure sums: examined[2] and skipped[2] by mate.  Per mate m, over all read groups: entered_m = the sum of
 * examined - skipped;  distinct_m = the number of sets;  largest_m = the reads of the largest set;  hist_m[i], i = 1 ... 256 = the sets
 * of i reads (bin 256: 256 and more).  distinct / entered is the share of reads that remains if deduplicated.
 * The list.  ppm is 10 ... 10^6 (the program's default 1000: FastQC's 0.1 %); the threshold is T_m = max(2, ceil(entered_m * ppm /
 * 10^6)) in 64-bit integer arithmetic (the product stays below 2^60).  Every set of mate m with count >= T_m is listed with its
 * sequence as letters, its count and a POSSIBLE SOURCE: the name of the first adapter of the adapter-by-cycle module's BUILT-IN set,
 * in the set's order, that occurs letter for letter in the listed sequence, else "-".  The list is sorted by mate, then count
 * descending, then sequence ascending as text.  The listed counts of a mate sum to at most entered_m, so at most floor(10^6 / ppm)
 * sets of a mate can be listed: the list's buffer has that size.
 * State.  A hash table in device memory of its own, the duplicate sets' kind: 24 bytes a slot, C = the smallest power of two >= 2
 * capacity (and >= 32) slots, capacity 16 ... 2^31 keys (the program's default 2^26: 3 GiB), and the per-lane sums.  NONE of it is part
 * of the flat state vector: bqc_state_words and every offset are the same with the module on, export and import carry none of it,
 * shards cannot be merged (a set may have members in two shards: --gpus N is refused by the program).  bqc_reset empties the table and
 * the sums and keeps the allocation.
 * Overflow.  When the reads hold more than `capacity` different keys (both mates together) the stream fails with BQC_ERR_RANGE where
 * other errors found on the card surface (a later submit, sync, flush or finalize); the message names the capacity and
 * --overrepresented-capacity.
 * bqc_enable_overrepresented switches the module on, after creation, in any order with the other enable calls (the ABI version stays
 * 2).  BQC_ERR_ARG, the message names the value: K outside 20 ... 56, ppm outside 10 ... 10^6, capacity outside 16 ... 2^31, in this
 * order.  BQC_ERR_STATE: a second call; a call after the context has taken a batch, has exported or imported state, or has been
 * finalised.  Without the call: no allocation, no launch.  With it: every other output is the same bytes as without it.
 * bqc_overrepresented: valid after bqc_finalize (which leaves the table as it is: it may be called again); the view is owned by the
 * context until the next finalize / destroy.  BQC_ERR_STATE: the module is off, or nothing has been finalised.
 * bqc_write_overrepresented: the text, lanes in the order of `hdr`, key-then-values lines:
 *   sample_id <id> / overrepresented_len <K> / overrepresented_ppm <ppm> / overrepresented_capacity <capacity> /
 *   lane <name> / sequence_reads_examined_first <n> / sequence_reads_examined_second <n> / sequence_reads_skipped_first <n> /
 *   sequence_reads_skipped_second <n>                                                                     (these five per read group)
 *   all_lanes / sequences_distinct_first <U> / sequence_set_largest_first <n> / sequence_set_size_histogram_first v1 ... v256 /
 *   overrepresented_threshold_first <T> / overrepresented_sequences_first <lines that follow> /
 *   <sequence> <count> <possible source or ->                                                             (one line per listed set)
 *   then the same five keys and the list with _second */
int bqc_enable_overrepresented(bqc_ctx* ctx, uint32_t prefix_len, uint32_t ppm, uint64_t capacity);
typedef struct bqc_ovr_seq {
    const char* seq;     /* the n letters of the set's key, as sequenced */
    uint64_t count;
    const char* source;  /* a built-in adapter's name, or "-" */
} bqc_ovr_seq;
typedef struct bqc_ovr_view {
    uint32_t prefix_len, ppm;
    uint64_t capacity;
    uint32_t n_lanes, pad;
    const uint64_t* lanes;              /* [n_lanes][4]: examined first, examined second, skipped first, skipped second */
    uint64_t distinct[2], largest[2];   /* [mate] */
    const uint64_t* hist[2];            /* [256]: sets of 1 ... 255 reads, of 256 and more */
    uint64_t threshold[2];
    uint32_t n_listed[2];
    const bqc_ovr_seq* listed[2];       /* [n_listed[m]], sorted */
} bqc_ovr_view;
int bqc_overrepresented(bqc_ctx* ctx, bqc_ovr_view* out);   /* after bqc_finalize */
int bqc_write_overrepresented(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path);

#ifdef __cplusplus
}
#endif
#endif /* BAMQC_H_ */
